"""Shared by tests/golden/make_flow_golden.py, tests/test_flow_golden.py and tests/test_gpu_flow_golden.py: the fixture of
a whole three-library run (tests/golden/flow_*.json.gz + flow_lib*.npz), captured from the reference's own loop body
(runBESST:160-218 with extend_paths off), and the loop that produces the same document from any implementation of it.

  * the assembly: contig sequences are cut out of a genome drawn by SHA-256 in counter mode (``genome_bytes``: no
    numpy bit generator that could drift), about a third of them stored reverse-complemented, some neighbours overlapping
    on the genome; a SHA-256 per contig is stored and checked, so a drifting generator is an error;
  * ``flip_records``: the records of a library as a mapper would report them against the flipped contigs;
  * ``run_pass`` / ``capture_*``: one pass of the loop body on an ``Api`` (the reference's modules or the package's) and
    what it leaves behind, as the JSON document the fixture stores per pass;
  * ``restore_state``: the object dicts and param fields a pass starts from, rebuilt from the stored state of the pass
    before it.
"""
import gzip
import hashlib
import io
import json
import os
import re

import numpy as np

from besst_amd.records import FLAG_MATE_REVERSE, FLAG_REVERSE, RecordBatch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SCENARIOS = ('flow_a', 'flow_b')
UNIQUE_ID = 1700000000
COLS = ('tid', 'mtid', 'pos', 'mpos', 'tlen', 'flag', 'mapq', 'qlen', 'rlen', 'alen')
ROWS_PER_FILE = 64000                    # records per flow_lib<k>_<part>.npz (keeps every file near 0.5 MB)
METRIC_FIELDS = ('read_len', 'mean_ins_size', 'std_dev_ins_size', 'ins_size_threshold', 'contig_threshold',
                 'skewness', 'skew_adj', 'contamination_ratio', 'contamination_mean', 'contamination_stddev',
                 'lognormal', 'lognormal_mean', 'lognormal_sigma')
GRAPH_FIELDS = ('mean_coverage', 'std_dev_coverage', 'edgesupport', 'expected_links_over_mean_plus_stddev',
                'scaffold_indexer', 'tot_assembly_length', 'current_N50', 'current_L50')
# per-library settings of a scenario that go to the parameter object (the CLI's -r -m -s -T -k -e)
LIB_FIELDS = ('read_len', 'mean_ins_size', 'std_dev_ins_size', 'ins_size_threshold', 'contig_threshold', 'edgesupport')
_COUNT_LINES = re.compile(r'^(\d+ isolated contigs removed from graph\.|\d+ cycles removed from graph\.|'
                          r'Nr of new scaffolds created in this step: \d+|\d+ link edges created\.|'
                          r'\(super\)Contigs after scaffolding: \d+|L50:.*)$')


# ---- sequences -----------------------------------------------------------------------------------------------------------
_COMPLEMENT = bytes.maketrans(b'ACGTacgtNn', b'TGCAtgcaNn')


def genome_bytes(tag, n):
    """n bases: SHA-256 of '<tag>/<counter>', two bits per base, most significant first, 0123 -> ACGT."""
    blocks = (int(n) + 127) // 128
    raw = np.frombuffer(b''.join(hashlib.sha256(('%s/%d' % (tag, i)).encode('ascii')).digest() for i in range(blocks)),
                        dtype=np.uint8)
    two = np.stack([(raw >> 6) & 3, (raw >> 4) & 3, (raw >> 2) & 3, raw & 3], axis=1).reshape(-1)[:int(n)]
    return np.frombuffer(b'ACGT', dtype=np.uint8)[two].tobytes()


def revcomp(seq):
    return seq.translate(_COMPLEMENT)[::-1]


def contig_starts(asm):
    lengths, gaps = np.asarray(asm['lengths'], np.int64), np.asarray(asm['gaps'], np.int64)
    return np.concatenate(([0], np.cumsum(lengths + gaps)[:-1]))


def contig_sequences(asm, check=True):
    """{name: sequence} of an assembly document.  A contig is its stretch of the genome (neighbours with a negative gap
    share bases), reverse-complemented where `flipped`, then edited (`edits`: [contig, from, to, 'lower' | 'N'] in stored
    coordinates).  With `check`, every sequence must have the stored SHA-256."""
    starts = contig_starts(asm)
    genome = genome_bytes(asm['genome_tag'], int(starts[-1]) + int(asm['lengths'][-1]))
    seqs = []
    for i, length in enumerate(asm['lengths']):
        s = genome[int(starts[i]):int(starts[i]) + int(length)]
        seqs.append(revcomp(s) if asm['flipped'][i] else s)
    for i, lo, hi, kind in asm['edits']:
        s = seqs[i]
        seqs[i] = s[:lo] + (s[lo:hi].lower() if kind == 'lower' else b'N' * (hi - lo)) + s[hi:]
    if check:
        for name, s, want in zip(asm['names'], seqs, asm['sha256']):
            if hashlib.sha256(s).hexdigest() != want:
                raise AssertionError('contig %s: the sequence generator no longer gives the stored sequence' % name)
    return {name: s.decode('ascii') for name, s in zip(asm['names'], seqs)}


def sequence_digests(asm):
    seqs = contig_sequences(asm, check=False)
    return [hashlib.sha256(seqs[n].encode('ascii')).hexdigest() for n in asm['names']]


# ---- records -------------------------------------------------------------------------------------------------------------
def _mate_rows(b):
    """Row of every record's mate: records keyed (tid, pos, mtid, mpos, read1) against (mtid, mpos, tid, pos, read2) of
    the others.  Exact duplicates share a key; they are matched in row order, which is a bijection among equal rows."""
    r1 = (b.flag & 0x40) != 0
    own = np.lexsort((r1, b.mpos, b.mtid, b.pos, b.tid))
    mate = np.lexsort((~r1, b.pos, b.tid, b.mpos, b.mtid))
    for x, y in (('tid', 'mtid'), ('pos', 'mpos')):
        assert np.array_equal(getattr(b, x)[own], getattr(b, y)[mate]), 'a record without its mate'
    assert np.array_equal(r1[own], ~r1[mate])
    out = np.zeros(len(b), np.int64)
    out[mate] = own
    return out


def flip_records(batch, flipped):
    """The stream a mapper would give had the contigs in `flipped` (bool per tid) been presented reverse-complemented:
    position from the other end (pos' = length - pos - alen, the aligned stretch keeps its extent), the read's own
    reverse flag on the reads of such a contig and the mate-reverse flag on their mates, mpos likewise, the sign of tlen
    for pairs inside the contig; then (tid, pos) order again (stable)."""
    flipped = np.asarray(flipped, bool)
    lengths = np.asarray(batch.lengths, np.int64)
    mate = _mate_rows(batch)
    alen = batch.alen.astype(np.int64)
    own_f, mate_f = flipped[batch.tid], flipped[batch.mtid]
    new_pos = np.where(own_f, lengths[batch.tid] - batch.pos - alen, batch.pos)
    assert (new_pos >= 0).all()
    cols = dict(tid=batch.tid, mtid=batch.mtid, pos=new_pos, mpos=new_pos[mate],
                tlen=np.where(own_f & (batch.tid == batch.mtid), -batch.tlen.astype(np.int64), batch.tlen),
                flag=batch.flag ^ (np.where(own_f, FLAG_REVERSE, 0) | np.where(mate_f, FLAG_MATE_REVERSE, 0)).astype(np.uint16),
                mapq=batch.mapq, qlen=batch.qlen, rlen=batch.rlen, alen=batch.alen)
    order = np.argsort((cols['tid'].astype(np.int64) << 32) | cols['pos'].astype(np.int64), kind='stable')
    return RecordBatch(batch.references, batch.lengths, **{k: np.asarray(v)[order] for k, v in cols.items()})


def save_library(k, batch, directory=GOLDEN_DIR):
    parts = range(0, len(batch), ROWS_PER_FILE)
    for p, lo in enumerate(parts):
        np.savez_compressed(os.path.join(directory, 'flow_lib%d_%d.npz' % (k, p)),
                            **{c: getattr(batch, c)[lo:lo + ROWS_PER_FILE] for c in COLS})
    return len(parts)


def load_library(k, n_parts, asm, directory=GOLDEN_DIR):
    cols = {c: [] for c in COLS}
    for p in range(n_parts):
        z = np.load(os.path.join(directory, 'flow_lib%d_%d.npz' % (k, p)))
        for c in COLS:
            cols[c].append(z[c])
    return RecordBatch(asm['names'], asm['lengths'], **{c: np.concatenate(v) for c, v in cols.items()})


# ---- documents -----------------------------------------------------------------------------------------------------------
def jsonable(o):
    if isinstance(o, dict):
        return {str(k): jsonable(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [jsonable(v) for v in o]
    if isinstance(o, np.integer):
        return int(o)
    if isinstance(o, np.floating):
        return float(o)
    if isinstance(o, np.bool_):
        return bool(o)
    return o


def write_doc(name, doc, directory=GOLDEN_DIR):
    with gzip.GzipFile(os.path.join(directory, name + '.json.gz'), 'wb', mtime=0) as gz, \
            io.TextIOWrapper(gz, encoding='ascii') as fh:
        json.dump(jsonable(doc), fh, separators=(',', ':'))


_docs = {}


def load_doc(name, directory=GOLDEN_DIR):
    if (name, directory) not in _docs:
        with gzip.open(os.path.join(directory, name + '.json.gz'), 'rt') as fh:
            _docs[(name, directory)] = json.load(fh)
    return _docs[(name, directory)]


def roundtrip(doc):
    """What the document reads back as (tuples become lists, keys strings)."""
    return json.loads(json.dumps(jsonable(doc)))


_libraries = {}


def load_inputs():
    """-> (assembly document, [RecordBatch per library]) - both scenarios run on the same records."""
    asm = load_doc('flow_assembly')
    if 'libs' not in _libraries:
        _libraries['libs'] = [load_library(k + 1, n, asm) for k, n in enumerate(asm['library_parts'])]
    return asm, _libraries['libs']


# ---- one implementation of the loop body ---------------------------------------------------------------------------------
class Api(object):
    """The modules a pass runs on.  `algorithm_and_output(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds,
    Information, param, pass_nr)` is runBESST:199-218: MakeScaffolds.Algorithm, every scaffold to F, PrintOutput."""

    def __init__(self, Parameter, Contig, Scaffold, get_metrics, PE, algorithm_and_output, after_pe=None):
        self.Parameter, self.Contig, self.Scaffold = Parameter, Contig, Scaffold
        self.get_metrics, self.PE, self.algorithm_and_output = get_metrics, PE, algorithm_and_output
        self.after_pe = after_pe                             # called with the library's records once PE is done


def package_api(store=None):
    """besst_amd's own loop body, as besst_amd.cli._run drives it."""
    from besst_amd import Contig, CreateGraph, Parameter, Scaffold, cli, libmetrics, session

    def algorithm_and_output(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, Information, param, pass_nr):
        cli.write_scaffolds(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, Information, param, pass_nr,
                            store)
    return Api(Parameter, Contig, Scaffold, libmetrics.get_metrics, CreateGraph.PE, algorithm_and_output,
               after_pe=session.close_session)


def new_param(api, scenario, out_dir):
    """The parameter object as runBESST:93-158 / besst_amd.cli._run fill it before the first library."""
    p = api.Parameter.parameter()
    p.scaffold_indexer = 1
    p.multiprocess = False
    p.no_score = False
    p.score_cutoff = 1.5
    p.max_extensions = None
    p.NO_ILP = False
    p.FASTER_ILP = False
    p.dfs_traversal = True
    p.print_scores = False
    p.development = False
    p.plots = False
    p.path_threshold = 100000
    p.hapl_ratio = 1.3
    p.hapl_threshold = 3
    p.detect_haplotype = False
    p.extend_paths = False
    p.first_lib = True
    p.min_mapq = 11
    p.lower_cov_cutoff = 0.001
    p.output_directory = out_dir
    p.information_file = io.StringIO()
    p.max_contig_overlap = scenario['max_contig_overlap']
    p.cov_cutoff = scenario['cov_cutoff']
    p.detect_duplicate = scenario['detect_duplicate']
    return p


def set_library(param, scenario, k, batch):
    lib = scenario['libraries'][k]
    param.pass_number = k + 1
    param.bamfile = 'lib%d.bam' % (k + 1)
    param.orientation = lib['orientation']
    for f in LIB_FIELDS:
        setattr(param, f, lib.get(f))
    param.contig_index = dict(enumerate(batch.references))


def edges_final(G):
    out = []
    for u, v in G.edges():
        d = G[u][v]
        if d['nr_links'] is None:
            continue
        row = dict(u=list(u), v=list(v), nr_links=d['nr_links'], obs=d['obs'], obs_sq=d['obs_sq'])
        for k in ('gap', 'score'):
            if k in d:
                row[k] = d[k]
        out.append(row)
    return out


def capture_after_pe(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, param):
    return dict(G=edges_final(G), G_prime=edges_final(G_prime),
                G_nodes=[list(n) for n in G.nodes()], G_prime_nodes=[list(n) for n in G_prime.nodes()],
                contigs=[[c.name, c.scaffold, c.coverage] for c in Contigs.values()],
                small_contigs=[[c.name, c.scaffold, c.coverage] for c in small_contigs.values()],
                scaffolds=list(Scaffolds.keys()), small_scaffolds=list(small_scaffolds.keys()),
                param={k: getattr(param, k, None) for k in GRAPH_FIELDS + ('no_score', 'contig_threshold')})


def capture_state(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, param):
    """What MakeScaffolds.Algorithm leaves, which is also what the next pass starts from (dict orders included)."""
    def contigs(d):
        return [[c.name, c.scaffold, c.position, bool(c.direction), c.length, c.coverage] for c in d.values()]

    def scaffolds(d):
        return [[key, s.name, [c.name for c in s.contigs], s.s_length] for key, s in d.items()]
    return dict(contigs=contigs(Contigs), small_contigs=contigs(small_contigs), scaffolds=scaffolds(Scaffolds),
                small_scaffolds=scaffolds(small_scaffolds), scaffold_indexer=param.scaffold_indexer,
                gap_estimations=list(param.gap_estimations), tot_assembly_length=param.tot_assembly_length,
                G_nodes=[list(n) for n in G.nodes()], G_prime_nodes=[list(n) for n in G_prime.nodes()])


def counting_lines(text):
    return [l for l in text.splitlines() if _COUNT_LINES.match(l)]


def fasta_summary(text):
    """Header lines, body lengths and a SHA-256 per body of a Scaffolds-pass<n>.fa (one body line per scaffold)."""
    lines = text.split('\n')
    assert lines[-1] == '' and len(lines) % 2 == 1
    heads, bodies = lines[0:-1:2], lines[1:-1:2]
    assert all(h.startswith('>') for h in heads)
    return dict(headers=heads, lengths=[len(b) for b in bodies],
                sha256=[hashlib.sha256(b.encode('ascii')).hexdigest() for b in bodies])


def capture_output(out_dir, pass_nr):
    pass_dir = os.path.join(out_dir, 'pass%d' % pass_nr)
    out = {}
    for key, fname in (('agp', 'info-pass%d.agp'), ('gff', 'info-pass%d.gff')):
        with open(os.path.join(pass_dir, fname % pass_nr), newline='') as fh:
            out[key] = fh.read()
    with open(os.path.join(pass_dir, 'Scaffolds-pass%d.fa' % pass_nr), newline='') as fh:
        out['fasta'] = fasta_summary(fh.read())
    return out


def run_pass(api, scenario, k, batch, param, state, C_dict, info):
    """Pass k + 1 (k from 0) of the loop body on `state` = (Contigs, Scaffolds, small_contigs, small_scaffolds), which it
    changes in place like the loop does.  -> the pass's document: metrics, after_pe, state, output, information."""
    Contigs, Scaffolds, small_contigs, small_scaffolds = state
    set_library(param, scenario, k, batch)
    mark = len(info.getvalue())
    merged_mark = len(param.information_file.getvalue())
    print('\nPASS ' + str(k + 1) + '\n\n', file=info)
    api.get_metrics(batch, param, info)
    doc = dict(metrics={f: getattr(param, f, None) for f in METRIC_FIELDS})
    G, G_prime = api.PE(Contigs, Scaffolds, info, C_dict, param, small_contigs, small_scaffolds, batch)
    if api.after_pe is not None:
        api.after_pe(batch)
    param.first_lib = False
    doc['after_pe'] = capture_after_pe(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, param)
    api.algorithm_and_output(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, info, param, k + 1)
    doc['state'] = capture_state(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, param)
    doc['output'] = capture_output(param.output_directory, k + 1)
    doc['information'] = counting_lines(info.getvalue()[mark:])
    doc['merging'] = [l for l in param.information_file.getvalue()[merged_mark:].splitlines() if l.startswith('merging ')]
    return roundtrip(doc)


def run_passes(api, scenario, asm, libs, out_dir, first=0, last=None, prev=None, observe=None):
    """Passes first + 1 .. last of the scenario (all by default), the state carried from pass to pass by the loop itself
    and never looked at in between.  `prev`: the stored document of pass `first` (None before the first pass), from whose
    state the run starts.  `observe(k, G, Scaffolds, small_scaffolds, param)` is called between PE and Algorithm.
    -> [pass documents]"""
    seqs = contig_sequences(asm)
    param = new_param(api, scenario, out_dir)
    info = io.StringIO()
    C_dict = dict(seqs) if first == 0 else {}                    # (InitializeObjects takes every contig out of C_dict)
    state = restore_state(api, asm, seqs, prev, param)
    inner = api.algorithm_and_output
    passes = []
    try:
        for k in range(first, len(libs) if last is None else last):
            if observe is not None:
                def wrapped(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, Information, p, pass_nr, k=k):
                    observe(k, G, Scaffolds, small_scaffolds, p)
                    inner(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, Information, p, pass_nr)
                api.algorithm_and_output = wrapped
            passes.append(run_pass(api, scenario, k, libs[k], param, state, C_dict, info))
    finally:
        api.algorithm_and_output = inner
    return passes


def restore_state(api, asm, seqs, prev, param):
    """(Contigs, Scaffolds, small_contigs, small_scaffolds) as the pass before left them (`prev` = its document), and the
    param fields that pass hands on: the loop keeps ONE parameter object, so whatever get_metrics does not set again for
    the next library (the skewness when -m is given, say) is still the last library's.  prev None: before the first pass."""
    if prev is None:
        return {}, {}, {}, {}
    for f, value in prev['metrics'].items():
        setattr(param, f, value)
    prev = prev['state']
    length = dict(zip(asm['names'], asm['lengths']))
    objs = {}
    dicts = []
    for key in ('contigs', 'small_contigs'):
        d = {}
        for name, scaf, pos, direction, clen, cov in prev[key]:
            assert clen == length[name]
            c = api.Contig.contig(name)
            c.scaffold, c.position, c.direction, c.length, c.coverage = scaf, pos, direction, clen, cov
            c.sequence = seqs[name]
            d[name] = objs[name] = c
        dicts.append(d)
    for key in ('scaffolds', 'small_scaffolds'):
        d = {}
        for dict_key, name, members, s_length in prev[key]:
            d[dict_key] = api.Scaffold.scaffold(name, [objs[m] for m in members], s_length)
        dicts.append(d)
    param.first_lib = False
    param.scaffold_indexer = prev['scaffold_indexer']
    param.gap_estimations = list(prev['gap_estimations'])
    param.tot_assembly_length = prev['tot_assembly_length']
    return dicts[0], dicts[2], dicts[1], dicts[3]


# ---- comparing a pass with the fixture -----------------------------------------------------------------------------------
def assert_scored_rows(got, want, doc, what, device):
    """Edge rows with `gap` and `score`.  Host paths run the restatement itself: tests/golden_util.assert_scored_rows.  The
    device's erf / exp are not libm's: structure and integer sums exactly; every gap exactly - the fixture script made
    sure that no edge of the run meets a near tie, so the reference's gap is the only admissible one -; every score within
    the tolerance of tests/golden_util.tolerances, which is far inside the spacing of the scores the script asserted."""
    from tests import golden_util as GU
    tol = GU.tolerances(doc)
    if not device or not tol['exact']:
        GU.assert_scored_rows(got, want, doc, what)
        return
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert {k: v for k, v in g.items() if k != 'score'} == {k: v for k, v in w.items() if k != 'score'}, (what, g, w)
        assert ('score' in g) == ('score' in w), (what, g, w)
        if 'score' in w:
            assert abs(g['score'] - w['score']) <= tol['score'], (what, g, w)


def assert_pass_equal(got, want, doc, what, device=False):
    """Every stored item of a pass: exactly, except `score` (and `gap` against fixtures made with the real mathstats
    package), see assert_scored_rows."""
    for key, value in want['metrics'].items():
        assert got['metrics'][key] == value, (what, 'metrics', key, got['metrics'][key], value)
    for key in ('G', 'G_prime'):
        assert_scored_rows(got['after_pe'][key], want['after_pe'][key], doc, '%s: after PE, %s' % (what, key), device)
    for key in want['after_pe']:
        if key not in ('G', 'G_prime'):
            assert got['after_pe'][key] == want['after_pe'][key], (what, 'after PE', key)
    for key in want['state']:
        assert got['state'][key] == want['state'][key], (what, 'after Algorithm', key)
    assert got['information'] == want['information'], (what, 'Information')
    assert got['merging'] == want['merging'], (what, 'merging lines')
    for key in ('agp', 'gff'):
        assert got['output'][key] == want['output'][key], (what, key)
    for key in ('headers', 'lengths', 'sha256'):
        assert got['output']['fasta'][key] == want['output']['fasta'][key], (what, 'FASTA', key)
    assert set(got) == set(want)


# ---- through the command line --------------------------------------------------------------------------------------------
def write_fasta(path, seqs):
    with open(path, 'w') as fh:
        for name, seq in seqs.items():
            fh.write('>%s\n' % name)
            fh.writelines(seq[i:i + 70] + '\n' for i in range(0, len(seq), 70))
    return path


def cli_args(scenario, fasta, bams, out):
    """The command line of a scenario -> (argv, per-library values that a command line cannot express).  -m -s -T -k -e -r
    take one value per library, and -r an integer: a scenario that sets them for one library only, with a fractional read
    length, is put into the parsed arguments."""
    argv = ['-c', fasta, '-f'] + bams + ['-orientation'] + [l['orientation'] for l in scenario['libraries']] + \
        ['-o', out, '--scaffolds', '-y', '-max_contig_overlap', str(scenario['max_contig_overlap'])]
    if not scenario['detect_duplicate']:
        argv.append('-d')
    if scenario['cov_cutoff'] is not None:
        argv += ['-z', str(scenario['cov_cutoff'])]
    dest = dict(read_len='readlen', mean_ins_size='mean', std_dev_ins_size='stddev', ins_size_threshold='threshold',
                contig_threshold='minsize', edgesupport='edgesupport')
    per_lib = {dest[f]: [l[f] for l in scenario['libraries']] for f in LIB_FIELDS
               if any(l[f] is not None for l in scenario['libraries'])}
    return argv, per_lib


def assert_files_equal_fixture(out_dir, doc, what, uid=None):
    for n, want in enumerate(doc['passes']):
        got = capture_output(out_dir, n + 1)
        if uid is not None:                                      # (another process's clock: the uid is its own)
            got['agp'], got['gff'] = (re.sub(r'_uid_\d+', '_uid_%d' % UNIQUE_ID, got[k]) for k in ('agp', 'gff'))
            got['fasta']['headers'] = [re.sub(r'_uid_\d+$', '_uid_%d' % UNIQUE_ID, h) for h in got['fasta']['headers']]
        for key in ('agp', 'gff'):
            assert got[key] == want['output'][key], (what, n + 1, key)
        for key in ('headers', 'lengths', 'sha256'):
            assert got['fasta'][key] == want['output']['fasta'][key], (what, n + 1, 'FASTA', key)
    with open(os.path.join(out_dir, 'Statistics.txt')) as fh:
        stats = fh.read()
    assert counting_lines(stats) == [l for p in doc['passes'] for l in p['information']], (what, 'Statistics.txt')
    assert [l for l in stats.splitlines() if l.startswith('merging ')] == [l for p in doc['passes'] for l in p['merging']]
