"""Thin command-line counterpart of ``runBESST`` for the accelerated path only.

    python -m besst_amd.cli -c contigs.fa -f lib1.bam [lib2.sam ...] -orientation fr [rf ...] -o outdir

Flag names and defaults follow runBESST:254-402 for everything the hot path reads (-m -s -T -k -r -e -z -z_min
--min_mapq -d -y --no_score -filter_contigs).  A ``-f`` file is a BAM or SAM text as an aligner prints it - plain, BGZF or
gzip, told by its content; the SAM lines are parsed on the GPU (bamio.ResidentSam), in any record order, and with
``--gzip_on_gpu`` a gzip SAM is inflated there too.  Per library it runs the BAM / SAM front-end, ``libmetrics.get_metrics`` and
``CreateGraph.PE`` and writes Statistics.txt plus the scored edge tables of G and G' as TSV.  With ``--scaffolds -y`` it
goes on like runBESST's loop without path extension: the graph is linearised, the paths become scaffolds, and every pass
writes ``pass<n>/Scaffolds-pass<n>.fa`` with its ``.agp`` and ``.gff`` (the sequence work on the GPU).  With
``--fasta_on_gpu`` the contig FASTA is parsed on the GPU into the sequence store instead of line by line in Python; a BGZF file is
inflated there as well, and with ``--gzip_on_gpu`` so is any other ``gzip`` file, of one member or of several (what the
device gives up on is read by zlib on the host, as without the flag).  With
``--outputs_on_gpu`` the AGP and GFF text is formatted on the GPU too, and ``repeats.fa`` / ``low_coverage_contigs.fa`` are
written from the sequence store in one go where the contigs live there (``--fasta_on_gpu``).  ``--final_fasta`` leaves the
directory as runBESST does without --separate_repeats: ``pass<n>/Scaffolds_pass<n>.fa`` holds the scaffolds followed by
the repeats, ``Scaffolds-pass<n>.fa`` and, after the last pass, ``repeats.fa`` are gone.  With ``--bgzf_outputs`` the
scaffold FASTA is compressed on the GPU and written as ``Scaffolds-pass<n>.fa.gz``, a BGZF file (what ``bgzip`` writes:
``samtools faidx`` and every gzip reader open it), and no ``.fa``; ``--final_fasta`` then leaves
``Scaffolds_pass<n>.fa.gz``, the repeats appended as further BGZF blocks.  AGP, GFF, ``repeats.fa``,
``low_coverage_contigs.fa`` and the TSVs stay plain.  With ``--bam_report`` every pass also counts what its BAM holds, in
one pass over the resident records on the GPU, and writes ``pass<n>/bam_report.tsv``, ``idxstats.tsv``, ``mapq_hist.tsv``,
``qlen_hist.tsv`` and ``insert_sizes.tsv`` (besst_amd.report).  With ``--assembly_report`` the contigs are counted on the
GPU before pass 1 - bases by class, lower case, runs of N: ``contig_report.tsv`` - and with ``--scaffolds`` every pass
writes ``pass<n>/scaffold_report.tsv`` for its scaffolds as written and ``pass<n>/assembly_stats.tsv`` (N50 / L50, gaps, GC:
contigs beside scaffolds; ``--report_min_gap N``: a run of N counts as a gap from N bases on; besst_amd.seqreport).  BESST's path
search (PROWithinScaf / PROBetweenScaf) stays with BESST - see INTEGRATION.md for plugging these calls into runBESST.

Several GPUs of one node: launch the same command line under torchrun, one process per GPU -

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m besst_amd.cli -c ... -f ...

Every rank ingests its slice of each BAM on its own GPU and takes part in the library scans and the graph build
(besst_amd.sharded); rank 0 writes the outputs.  The sharded input is BAM: a SAM file is refused there.
"""
from __future__ import print_function

import argparse
import gzip
import os
import shutil
import sys
from time import time

from . import CreateGraph as CG
from . import GenerateOutput as GO
from . import MakeScaffolds as MS
from . import Parameter, bamio, libmetrics, mathstats_compat, report, seqreport, session


def open_fasta(path):
    """The contig FASTA as text; a file that begins with the gzip magic (gzip, bgzip, --bgzf_outputs) through gzip."""
    with open(path, 'rb') as fh:
        magic = fh.read(2)
    return gzip.open(path, 'rt') if magic == b'\x1f\x8b' else open(path)


def read_fasta(path):
    seqs, name, chunks = {}, None, []
    with open_fasta(path) as fh:
        for line in fh:
            if line.startswith('>'):
                if name is not None:
                    seqs[name] = ''.join(chunks)
                name, chunks = line[1:].strip().split()[0], []
            else:
                chunks.append(line.strip())
    if name is not None:
        seqs[name] = ''.join(chunks)
    return seqs


def build_parser():
    ap = argparse.ArgumentParser(prog='besst_amd.cli', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('-c', dest='contigfile', required=True,
                    help='contig FASTA, plain or gzip / BGZF compressed (told by its first bytes, not its name)')
    ap.add_argument('-f', dest='bamfiles', nargs='+', required=True,
                    help='one BAM or SAM file per library (SAM text plain, BGZF or gzip; told by content, not by name; every form is '
                         'streamed in chunks, so a compressed SAM may be of any size - BGZF is inflated on the GPU)')
    ap.add_argument('-o', dest='output', default='.', help='output directory')
    ap.add_argument('-orientation', dest='orientation', nargs='+', choices=['fr', 'rf'], required=True)
    ap.add_argument('-r', dest='readlen', type=int, nargs='+')
    ap.add_argument('-m', dest='mean', type=float, nargs='+')
    ap.add_argument('-s', dest='stddev', type=float, nargs='+')
    ap.add_argument('-T', dest='threshold', type=int, nargs='+')
    ap.add_argument('-k', dest='minsize', type=int, nargs='+')
    ap.add_argument('-e', dest='edgesupport', type=int, nargs='+')
    ap.add_argument('-z', dest='covcutoff', type=int, default=None)
    ap.add_argument('-z_min', dest='lower_covcutoff', type=float, default=0.001)
    ap.add_argument('--min_mapq', dest='min_mapq', type=int, default=11)
    ap.add_argument('-d', dest='duplicate', action='store_false', help='switch duplicate detection off')
    ap.add_argument('-y', dest='extendpaths', action='store_false', help='switch path extension off')
    ap.add_argument('--no_score', dest='no_score', action='store_true')
    ap.add_argument('-max_contig_overlap', dest='max_contig_overlap', type=int, default=200,
                    help='longest overlap between neighbouring contig ends that is looked for when scaffolds are written')
    ap.add_argument('--scaffolds', action='store_true',
                    help='per pass: linearise the graph, chain the paths into scaffolds (MakeScaffolds.Algorithm without '
                         'path extension) and write Scaffolds-pass<n>.fa, info-pass<n>.agp and info-pass<n>.gff; needs -y '
                         'and scoring')
    ap.add_argument('--fasta_on_gpu', dest='fasta_on_gpu', action='store_true',
                    help='read the contig FASTA on the GPU: the file goes to HBM as it is and is parsed there into the '
                         'sequence store (GenerateOutput.SequenceStore.from_fasta); the sequences do not pass through '
                         'Python strings.  A BGZF file (bgzip, --bgzf_outputs) is inflated on the GPU too; any other gzip '
                         'file by zlib on the host')
    ap.add_argument('--gzip_on_gpu', dest='gzip_on_gpu', action='store_true',
                    help="with --fasta_on_gpu: a contig FASTA that is gzip but not BGZF (gzip's own output; one member or "
                         'several, as cat, gzip -c >> and multi-member compressors leave them) is inflated on '
                         'the GPU as well - block starts found by probing, chunks decoded side by side, CRC-32 checked; what '
                         'the GPU does not take is read by zlib on the host as without the flag; needs --fasta_on_gpu.  '
                         'It applies to a gzip-compressed SAM file of -f in the same way, with or without --fasta_on_gpu')
    ap.add_argument('--outputs_on_gpu', dest='outputs_on_gpu', action='store_true',
                    help='format info-pass<n>.agp / .gff on the GPU, and write repeats.fa / low_coverage_contigs.fa '
                         'from the sequence store in one go where the contigs live there (--fasta_on_gpu)')
    ap.add_argument('--final_fasta', dest='final_fasta', action='store_true',
                    help="leave runBESST's final files: pass<n>/Scaffolds_pass<n>.fa = the scaffolds followed by "
                         'repeats.fa (Scaffolds-pass<n>.fa is renamed, repeats.fa removed after the last pass); needs '
                         '--scaffolds')
    ap.add_argument('--bgzf_outputs', dest='bgzf_outputs', action='store_true',
                    help='write Scaffolds-pass<n>.fa.gz instead of .fa: BGZF (bgzip) blocks, compressed on the GPU from the '
                         'buffer the FASTA is produced in (with --final_fasta: Scaffolds_pass<n>.fa.gz); needs --scaffolds')
    ap.add_argument('-filter_contigs', dest='contig_filter_length', type=int, default=None,
                    help='leave contigs shorter than this out of the run (runBESST -filter_contigs)')
    ap.add_argument('--threads', type=int, default=None, help='BAM inflate threads')
    ap.add_argument('--bam_report', dest='bam_report', action='store_true',
                    help='per pass, count what the BAM holds in one pass over the resident records on the GPU and write '
                         'pass<n>/bam_report.tsv (the rows of samtools flagstat, the pair classes, a digest of the columns), '
                         'idxstats.tsv (the numbers of samtools idxstats), mapq_hist.tsv, qlen_hist.tsv and insert_sizes.tsv; '
                         'the census goes to Statistics.txt too, with a note when the pairs speak against -orientation or '
                         "the contig lengths against the header's")
    ap.add_argument('--assembly_report', dest='assembly_report', action='store_true',
                    help='count what the contigs hold on the GPU - bases by class, lower case, runs of N - and write '
                         'contig_report.tsv, one row per contig, before pass 1; with --scaffolds every pass also writes '
                         'pass<n>/scaffold_report.tsv for its scaffolds as written and pass<n>/assembly_stats.tsv (N50 / L50, '
                         'N90 / L90, auN, GC, gaps: contigs beside scaffolds), and the before -> after lines go to '
                         'Statistics.txt.  Contigs that hold a byte the scaffold writer has no complement for are named')
    ap.add_argument('--report_min_gap', dest='report_min_gap', type=int, default=1, metavar='N',
                    help='with --assembly_report: a run of N counts as a gap from this many bases on (default 1)')
    ap.add_argument('--linearize', action='store_true',
                    help="also run steps 1-4 of MakeScaffolds.Algorithm on a copy of G (isolated scaffolds, "
                         "score-based ambiguity removal, cycles) and write the surviving link edges")
    return ap


def _input_format(path):
    """'bam', 'sam' or 'sam.gz' (SAM text behind the gzip magic) of a -f file; a file that cannot be read counts as 'bam':
    opening it says what is wrong."""
    try:
        fmt = bamio.sniff_format(path)
        if fmt == 'sam':
            with open(path, 'rb') as fh:
                if fh.read(2) == bamio.GZIP_MAGIC:
                    return 'sam.gz'
        return fmt
    except OSError:
        return 'bam'


def _per_lib(values, i):
    return values[i] if values is not None else None


def write_edges(path, G):
    with open(path, 'w') as fh:
        print('scaffold1\tside1\tscaffold2\tside2\tnr_links\tobs\tobs_sq\tgap\tscore', file=fh)
        for u, v in G.edges():
            d = G[u][v]
            if d['nr_links'] is None:
                continue
            print('\t'.join(str(x) for x in (u[0], u[1], v[0], v[1], d['nr_links'], d['obs'], d['obs_sq'],
                                             d.get('gap', ''), d.get('score', ''))), file=fh)


def write_scaffolds(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, Information, param, pass_nr, store):
    """MakeScaffolds.Algorithm with extend_paths off (MakeScaffolds.py:66-90) on the pass's own graphs and dicts - the
    next library sees the new contig table - then runBESST:205-218: every scaffold to F, F to the three output files."""
    t0 = time()
    # the two lines Algorithm opens with (MakeScaffolds.py:51-57)
    print(str(sum(1 for u, v in G.edges() if G[u][v]['nr_links'])) + ' link edges created.', file=Information)
    print('Perform inference on scaffold graph...', file=Information)
    dValuesTable = None
    if param.std_dev_ins_size:
        dValuesTable = mathstats_compat.PreCalcMLvaluesOfdLongContigs(param.mean_ins_size, param.std_dev_ins_size,
                                                                      param.read_len)
    G, Contigs, Scaffolds = MS.LinearizeGraph(G, G_prime, Contigs, Scaffolds, Information, param)
    MS.NewContigsScaffolds(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, Information, dValuesTable, param,
                           set())
    print('Time elapsed for making scaffolds, iteration ' + str(pass_nr - 1) + ': ' + str(time() - t0) + '\n',
          file=Information)
    t0 = time()
    F = []
    for scaffold_ in small_scaffolds:
        F = GO.WriteToF(F, small_contigs, small_scaffolds[scaffold_].contigs)
    for scaffold_ in Scaffolds:
        F = GO.WriteToF(F, Contigs, Scaffolds[scaffold_].contigs)
    GO.PrintOutput(F, Information, param.output_directory, param, pass_nr, store=store)
    print('Time elapsed for writing the scaffolds, iteration ' + str(pass_nr - 1) + ': ' + str(time() - t0) + '\n',
          file=Information)


def write_contig_report(store, C_dict, param, out, Information, min_gap, per_pass):
    """--assembly_report, before pass 1: the census of the run's contigs (the rows of the filtered ``C_dict``) from the
    store as BESST_output/contig_report.tsv, the baseline column of every pass's assembly_stats.tsv, and one warning line -
    stderr and Statistics.txt - that names up to ten contigs holding a byte the scaffold writer has no complement for."""
    t0 = time()
    census = store.report(rows=[store.index[name] for name in C_dict], min_gap=min_gap).finalised()
    census.write(os.path.join(out, 'contig_report.tsv'))
    param.contig_stats = stats = seqreport.AssemblyStats(census)
    param.report_min_gap = min_gap
    param.assembly_report = per_pass                              # PrintOutput writes the per-pass files
    print('Assembly report of the contigs (contig_report.tsv): %d sequences, %d bases, N50 %s, L50 %s, %d gaps, %d N, '
          'counted in %s s' % (stats.n, stats.total, stats.N50, stats.L50, stats.gaps, stats.n_bases, time() - t0),
          file=Information)
    odd = [name for name, other in zip(census.names, census.other.tolist()) if other > 0]
    if odd:
        line = ('WARNING: %d contig(s) hold a byte that is no base, N or IUPAC code (%s%s): a pass that writes one of them '
                'reversed stops with the KeyError of that byte, as BESST does' % (
                    len(odd), ', '.join(odd[:10]), ', ...' if len(odd) > 10 else ''))
        print(line, file=sys.stderr)
        print(line, file=Information)


def write_bam_report(records, param, C_dict, pass_dir, Information, lead):
    """--bam_report: the report of the opened BAM (every rank takes part under a process group; rank 0 writes) as files
    in the pass's directory, the census in Statistics.txt, and the two notes - the pairs against the named orientation, the
    FASTA's contig lengths against the header's.  The run goes on unchanged."""
    t0 = time()
    rep = records.report()
    if not lead:
        return
    rep.write(pass_dir)
    print('BAM report of %s (pass%d/bam_report.tsv, idxstats.tsv, mapq_hist.tsv, qlen_hist.tsv, insert_sizes.tsv):'
          % (param.bamfile, param.pass_number), file=Information)
    for line in rep.census_lines():
        print(line, file=Information)
    note = report.orientation_note(rep, param.orientation)
    if note:
        print(note, file=sys.stderr)
        print(note, file=Information)
    bad = report.length_mismatches(records.references, records.lengths, {name: len(seq) for name, seq in C_dict.items()})
    if bad:
        text = ('NOTE: %d contig(s) have another length in the contig file than in the header of %s (was it mapped to '
                'another contig file?): %s' % (len(bad), param.bamfile,
                                               ', '.join('%s (%d, header %d)' % (n, fl, hl) for n, hl, fl in bad[:10])))
        print(text, file=sys.stderr)
        print(text, file=Information)
    print('Time elapsed for the BAM report, iteration ' + str(param.pass_number - 1) + ': ' + str(time() - t0) + '\n',
          file=Information)


def finish_pass_fasta(out, pass_nr, bgzf=False):
    """runBESST:220-226: Scaffolds-pass<n>.fa becomes Scaffolds_pass<n>.fa, followed by repeats.fa as it stands now (the
    scaffolds are renamed and the repeats appended: the large file is not copied).  ``bgzf``: the same for the pass's
    .fa.gz - its EOF block is cut off, the repeats follow as BGZF blocks from the same compressor, then one EOF block."""
    pass_dir = os.path.join(out, 'pass%d' % pass_nr)
    ext = '.fa.gz' if bgzf else '.fa'
    final = os.path.join(pass_dir, 'Scaffolds_pass%d%s' % (pass_nr, ext))
    os.replace(os.path.join(pass_dir, 'Scaffolds-pass%d%s' % (pass_nr, ext)), final)
    repeats = os.path.join(out, 'repeats.fa')
    if bgzf:
        eof = GO.BGZF_EOF
        with open(final, 'r+b') as dst:
            size = dst.seek(0, os.SEEK_END)
            if size < len(eof):
                raise IOError('%s does not end with the BGZF EOF block' % final)
            dst.seek(size - len(eof))
            if dst.read(len(eof)) != eof:
                raise IOError('%s does not end with the BGZF EOF block' % final)
            dst.truncate(size - len(eof))
            dst.seek(size - len(eof))
            if os.path.exists(repeats):
                step = GO.bgzf_chunk(64 << 20)                  # whole blocks: only the file's last block is short
                with open(repeats, 'rb') as src:
                    while True:
                        data = src.read(step)
                        if not data:
                            break
                        dst.write(GO.bgzf_compress(data, eof=False))
            dst.write(eof)
    elif os.path.exists(repeats):
        with open(final, 'ab') as dst, open(repeats, 'rb') as src:
            shutil.copyfileobj(src, dst, 16 << 20)
    return final


def join_process_group():
    """Under torchrun (WORLD_SIZE > 1): one rank per GPU over RCCL (backend 'nccl'; BESST_DIST_BACKEND=gloo for several
    ranks on one GPU).  -> (rank, whether this call initialised the group)."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world < 2:
        return 0, False
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')) % max(1, torch.cuda.device_count()))
    from . import sharded
    if dist.is_initialized():
        sharded.enable()
        return dist.get_rank(), False
    # a rank that never arrives ends the job instead of holding it: every collective gives up after this long (gloo raises
    # in the waiting ranks; under RCCL the watchdog tears the process down)
    import datetime
    limit = datetime.timedelta(seconds=float(os.environ.get('BESST_COLLECTIVE_TIMEOUT', '1800')))
    dist.init_process_group(os.environ.get('BESST_DIST_BACKEND', 'nccl'), timeout=limit)
    sharded.enable()                                         # every rank makes the drop-in's calls together from here on
    return dist.get_rank(), True


def main(argv=None):
    args = build_parser().parse_args(argv)
    if len(args.orientation) != len(args.bamfiles):
        sys.exit('need one -orientation per BAM file')
    if args.scaffolds and args.extendpaths:
        sys.exit('--scaffolds needs -y: with path extension on, BESST places contigs with its path search '
                 '(PROWithinScaf / PROBetweenScaf), which is not part of this package - the scaffolds would not be BESST\'s')
    if args.scaffolds and args.no_score:
        sys.exit('--scaffolds cannot be combined with --no_score: without scores BESST skips the linearisation and the '
                 'scaffold step, and its path search, which would do the work instead, is not part of this package')
    if args.final_fasta and not args.scaffolds:
        sys.exit('--final_fasta needs --scaffolds: Scaffolds_pass<n>.fa is the scaffold FASTA followed by the repeats')
    if args.bgzf_outputs and not args.scaffolds:
        sys.exit('--bgzf_outputs needs --scaffolds: the file it compresses is the scaffold FASTA')
    formats = [_input_format(path) for path in args.bamfiles]
    if args.gzip_on_gpu and not args.fasta_on_gpu and 'sam.gz' not in formats:
        sys.exit('--gzip_on_gpu needs --fasta_on_gpu: it is the sequence store that reads the compressed file on the GPU')
    if args.max_contig_overlap < 0 or args.max_contig_overlap > GO.MAX_CONTIG_OVERLAP_LIMIT:
        sys.exit('-max_contig_overlap must lie in 0..%d' % GO.MAX_CONTIG_OVERLAP_LIMIT)
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        for path, fmt in zip(args.bamfiles, formats):
            if fmt in ('sam', 'sam.gz'):                         # every rank alike, before any collective
                sys.exit(bamio.SHARDED_SAM_MESSAGE % path)
    rank, joined = join_process_group()
    try:
        return _run(args, rank)
    finally:
        if joined:
            import torch.distributed as dist
            dist.destroy_process_group()


def _run(args, rank):
    out = os.path.join(args.output, 'BESST_output')
    os.makedirs(out, exist_ok=True)
    lead = rank == 0                                         # the followers compute, rank 0 also writes
    param = Parameter.parameter()
    param.scaffold_indexer = 1
    param.min_mapq = args.min_mapq
    param.cov_cutoff = args.covcutoff
    param.lower_cov_cutoff = args.lower_covcutoff
    param.no_score = args.no_score
    param.detect_duplicate = args.duplicate
    param.extend_paths = args.extendpaths
    param.detect_haplotype = False
    param.print_scores = False
    param.max_contig_overlap = args.max_contig_overlap
    param.outputs_on_gpu = args.outputs_on_gpu
    param.outputs_bgzf = args.bgzf_outputs
    param.output_directory = out
    param.first_lib = True
    Information = param.information_file = open(os.path.join(out, 'Statistics.txt') if lead else os.devnull, 'w')
    fasta_on_gpu, filter_length = args.fasta_on_gpu, args.contig_filter_length
    if fasta_on_gpu:
        # file bytes -> HBM -> the store; C_dict holds handles into it (the filtered contigs stay in the pool, unused)
        store = GO.SequenceStore.from_fasta(args.contigfile, gzip_on_gpu=args.gzip_on_gpu) if lead else None
        C_dict = store.contig_dict(filter_length, Information) if lead else {}
        if lead and args.outputs_on_gpu:
            store.batch_fasta = True
    else:
        C_dict = read_fasta(args.contigfile) if lead else {}
        if lead and filter_length is not None:
            GO.filter_contigs(C_dict, filter_length, Information)
    if lead:
        print('Number of initial contigs:', len(C_dict))
    Contigs, Scaffolds, small_contigs, small_scaffolds = {}, {}, {}, {}
    if not fasta_on_gpu:
        # the sequences go to the GPU once, before CreateGraph.PE drops repeats and low-coverage contigs from its dicts
        store = GO.SequenceStore(list(C_dict), list(C_dict.values())) if (args.scaffolds or args.assembly_report) and lead else None
        if store is not None and args.outputs_on_gpu:
            store.batch_fasta = True
    if args.assembly_report and lead:
        write_contig_report(store, C_dict, param, out, Information, args.report_min_gap, bool(args.scaffolds))
    for i, bam in enumerate(args.bamfiles):
        param.pass_number = i + 1
        param.bamfile = bam
        param.orientation = args.orientation[i]
        param.mean_ins_size = _per_lib(args.mean, i)
        param.std_dev_ins_size = _per_lib(args.stddev, i)
        param.ins_size_threshold = _per_lib(args.threshold, i)
        param.contig_threshold = _per_lib(args.minsize, i)
        param.edgesupport = _per_lib(args.edgesupport, i)
        param.read_len = _per_lib(args.readlen, i)
        print('\nPASS ' + str(i + 1) + '\n\n', file=Information)
        t0 = time()
        # straight to HBM: inflate + record decode on the GPU (any BGZF block layout)
        # (under torchrun: this rank's slice of the file, on this rank's GPU)
        # (--gzip_on_gpu also applies to a gzip SAM; the keyword goes along only when the flag is given)
        records = bamio.open_bam(bam, threads=args.threads, **({'gzip_on_gpu': True} if args.gzip_on_gpu else {}))
        print('Time elapsed reading %s (%d records): %s' % (bam, len(records), time() - t0), file=Information)
        param.contig_index = dict(enumerate(records.references))
        if args.bam_report:
            write_bam_report(records, param, C_dict, os.path.join(out, 'pass%d' % (i + 1)), Information, lead)
        t0 = time()
        libmetrics.get_metrics(records, param, Information)
        print('Time elapsed for getting libmetrics, iteration ' + str(i) + ': ' + str(time() - t0) + '\n',
              file=Information)
        t0 = time()
        G, G_prime = CG.PE(Contigs, Scaffolds, Information, C_dict, param, small_contigs, small_scaffolds, records)
        print('Total time for CreateGraph-module, iteration ' + str(i) + ': ' + str(time() - t0) + '\n',
              file=Information)
        session.close_session(records)
        records.close()
        param.first_lib = False
        if not lead:
            continue
        pass_dir = os.path.join(out, 'pass%d' % (i + 1))
        os.makedirs(pass_dir, exist_ok=True)
        write_edges(os.path.join(pass_dir, 'edges_G.tsv'), G)
        write_edges(os.path.join(pass_dir, 'edges_Gprime.tsv'), G_prime)
        if args.linearize and not param.no_score:
            # on copies: the graphs CreateGraph.PE returned stay as BESST's own MakeScaffolds expects them
            t0 = time()
            L, L_prime = G.copy(), G_prime.copy()
            L, _, _ = MS.LinearizeGraph(L, L_prime, Contigs, Scaffolds, Information, param)
            print('Time elapsed for the graph linearisation (steps 1-4), iteration ' + str(i) + ': ' + str(time() - t0)
                  + '\n', file=Information)
            write_edges(os.path.join(pass_dir, 'edges_G_linear.tsv'), L)
        if args.scaffolds:
            write_scaffolds(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, Information, param, i + 1, store)
            if args.final_fasta:
                finish_pass_fasta(out, i + 1, bgzf=args.bgzf_outputs)
        print('pass %d: %d records, G %d link edges, G_prime %d link edges' % (
            i + 1, len(records), sum(1 for u, v in G.edges() if G[u][v]['nr_links'] is not None),
            sum(1 for u, v in G_prime.edges() if G_prime[u][v]['nr_links'] is not None)))
    if lead and args.final_fasta and os.path.exists(os.path.join(out, 'repeats.fa')):
        os.remove(os.path.join(out, 'repeats.fa'))               # runBESST:233-234
    if store is not None:
        store.close()
    Information.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
