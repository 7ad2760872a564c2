"""The assembly report above the census kernel: ``census_store`` on the contig pool, ``ScaffoldEmitter.report`` on the
scaffolds as emitted (every case of the fixture captured from the reference, in windows of several sizes), ``PrintOutput``
with and without ``param.assembly_report``, and ``cli --assembly_report`` end to end.  The reference throughout is the
tests' own model (tests/seq_census_model.py) over the FASTA text, split at its headers in plain Python."""
import gzip
import io
import os

import numpy as np
import pytest

from besst_amd import GenerateOutput as GO
from besst_amd import seqreport
from tests import output_util as OU
from tests import seq_census_model as M

pytestmark = pytest.mark.gpu

DOC = OU.load_golden()
CASES = {c['name']: c for c in DOC['cases']}
UID = DOC['unique_id']
GOOD = sorted(n for n, c in CASES.items() if c['expect']['key_error'] is None)
BAD = sorted(n for n, c in CASES.items() if c['expect']['key_error'] is not None)


def _param(case, out_dir=None, **extra):
    param = OU.Param(case['K'], case['sigma'], None if out_dir is None else str(out_dir), io.StringIO())
    for key, value in extra.items():
        setattr(param, key, value)
    return param


def model_rows(fasta_bytes, min_gap=1):
    """[(name, partial census)] of a FASTA text"""
    return [(name, M.partial(seq, min_gap)) for name, seq in M.split_fasta(fasta_bytes)]


CONTIGS = [('plain', 'ACGTACGTTTGACCA'), ('lower_iupac', 'acgtNNNNryKMacgtnnX'), ('twice', 'NNNNACGT'), ('empty', ''),
           ('odd', 'ACG*TU-x'), ('twice', 'GGGGCCCCNN'), ('all_n', 'N' * 37), ('long', 'ACGTN' * 4000 + 'acgt')]


def test_census_store_from_strings_and_from_fasta(tmp_path):
    names, seqs = [n for n, _ in CONTIGS], [s for _, s in CONTIGS]
    want = [M.partial(s.encode()) for s in seqs]
    path = str(tmp_path / 'contigs.fa')
    with open(path, 'w') as fh:
        for n, s in CONTIGS:
            fh.write('>%s\n%s\n' % (n, '\n'.join(s[k:k + 70] for k in range(0, len(s), 70))))
    with GO.SequenceStore(names, seqs) as store, GO.SequenceStore.from_fasta(path) as parsed:
        for st in (store, parsed):
            census = st.report()
            assert census.names == names and not census.final
            assert census.words.tolist() == want
            assert census.finalised().words.tolist() == [M.whole(s.encode()) for s in seqs]
            assert census.other.tolist() == [0, 0, 0, 0, 4, 0, 0, 0] and census.lower[1] == 12
            rows = [6, 1, 1, 5]                                  # a subset, in any order, a row twice, the duplicate name
            part = seqreport.census_store(st, rows, min_gap=4)
            assert part.names == [names[r] for r in rows]
            assert part.words.tolist() == [M.partial(seqs[r].encode(), 4) for r in rows]
            assert part.finalised().gaps.tolist() == [1, 1, 1, 0]
            with pytest.raises(ValueError):
                st.report(rows=[len(names)])


@pytest.mark.parametrize('name', GOOD)
def test_emitter_report_equals_the_model_over_the_expected_fasta(name):
    case = CASES[name]
    text = case['expect']['fasta'].encode('ascii')
    want = model_rows(text)
    for window in (16, 48, 4096, None):
        em = GO.ScaffoldEmitter(OU.case_F(case), _param(case), None, UID)
        try:
            census = em.report(window_bytes=window)
            seq_off, seq_len = em.sequence_ranges()
        finally:
            em.close()
        assert census.names == [n for n, _ in want]
        assert census.words.tolist() == [w for _, w in want], (name, window)
        assert census.length.tolist() == [len(seq) for _, seq in M.split_fasta(text)] == seq_len.tolist()
        assert [text[o:o + n] for o, n in zip(seq_off.tolist(), seq_len.tolist())] == [seq for _, seq in M.split_fasta(text)]
    assert census.finalised().words.tolist() == [M.whole(seq) for _, seq in M.split_fasta(text)]


@pytest.mark.parametrize('name', BAD)
def test_a_key_error_of_the_reference_is_raised_by_report(name):
    case = CASES[name]
    param = _param(case)
    em = GO.ScaffoldEmitter(OU.case_F(case), param, None, UID)
    try:
        with pytest.raises(KeyError) as exc:
            em.report(window_bytes=48)
        assert exc.value.args == (case['expect']['key_error'],)
    finally:
        em.close()
    assert param.information_file.getvalue() == ''              # the `merging` lines are PrintOutput's to print


def test_emitter_report_on_a_seeded_assembly():
    asm = OU.seeded_assembly(400, 50, 3000, 23)
    want_text = OU.numpy_fasta(asm['scaffolds'], asm['pool'], asm['offsets'], asm['lengths'], asm['overlaps'], asm['sigma'],
                               UID).tobytes()
    want = model_rows(want_text, 30)
    assert sum(w[M.RUNS] for _, w in want) > 50 and len(asm['overlaps']) >= 2
    param = OU.Param(200, asm['sigma'], None, io.StringIO())
    with OU.store_of(asm) as store:
        em = GO.ScaffoldEmitter(asm['F'], param, store, UID)
        try:
            for window in (4096 + 48, None):
                census = em.report(window_bytes=window, min_gap=30)
                assert census.names == [n for n, _ in want] and census.words.tolist() == [w for _, w in want]
            merged = int(em.layout.drop.sum())
        finally:
            em.close()
        contigs = store.report()
    assert merged > 0
    # every base of the contigs is in the scaffolds but the merged ones; what was added is 'n' and 'N'
    total = census.words.sum(axis=0)
    assert int(total[M.LEN] - total[M.N]) == int(contigs.length.sum()) - merged


def test_print_output_writes_the_report_and_nothing_else_changes(tmp_path):
    case = CASES['short_K200'] if 'short_K200' in CASES else CASES[GOOD[0]]
    text = case['expect']['fasta'].encode('ascii')
    off_dir, on_dir = tmp_path / 'off', tmp_path / 'on'
    off_dir.mkdir(); on_dir.mkdir()
    info_off, info_on = io.StringIO(), io.StringIO()
    p_off = _param(case, off_dir)
    GO.PrintOutput(OU.case_F(case), info_off, str(off_dir), p_off, 1, unique_id=UID)
    baseline = seqreport.AssemblyStats(seqreport.SequenceCensus(
        ['c%d' % k for k in range(3)], np.asarray([M.partial(b'ACGT' * 10), M.partial(b'ACNNGT'), M.partial(b'A')])))
    p_on = _param(case, on_dir, assembly_report=True, contig_stats=baseline, report_min_gap=2)
    GO.PrintOutput(OU.case_F(case), info_on, str(on_dir), p_on, 1, unique_id=UID)
    plain = sorted(os.listdir(str(off_dir / 'pass1')))
    assert sorted(os.listdir(str(on_dir / 'pass1'))) == sorted(plain + ['assembly_stats.tsv', 'scaffold_report.tsv'])
    for fname in plain:                                          # the flag changes no file of the parent behaviour
        with open(str(off_dir / 'pass1' / fname), 'rb') as a, open(str(on_dir / 'pass1' / fname), 'rb') as b:
            assert a.read() == b.read(), fname
    with open(str(on_dir / 'pass1' / 'Scaffolds-pass1.fa'), 'rb') as fh:
        assert fh.read() == text
    assert p_on.information_file.getvalue() == p_off.information_file.getvalue()       # `merging` lines once
    # flag absent or false: exactly today's lines; flag on: the same lines first, then the report's
    assert info_off.getvalue() == case['expect']['information']
    p_false = _param(case, tmp_path / 'off', assembly_report=False)
    info_false = io.StringIO()
    GO.PrintOutput(OU.case_F(case), info_false, str(off_dir), p_false, 1, unique_id=UID)
    assert info_false.getvalue() == info_off.getvalue() and sorted(os.listdir(str(off_dir / 'pass1'))) == plain
    assert info_on.getvalue().startswith(info_off.getvalue())
    lines = info_on.getvalue()[len(info_off.getvalue()):].splitlines()
    back = seqreport.SequenceCensus.read(str(on_dir / 'pass1' / 'scaffold_report.tsv'))
    want = model_rows(text, 2)
    assert back.names == [n for n, _ in want] and back.min_gap == 2
    assert back.words.tolist() == [M.finalise(w, 2) for _, w in want]
    stats = seqreport.AssemblyStats(back)
    lengths = [w[M.LEN] for _, w in want]
    assert (stats.N50, stats.L50) == (M.nx(lengths, 50), M.lx(lengths, 50))
    assert lines[0] == 'Assembly report: N50 %d -> %d, L50 %d -> %d' % (baseline.N50, stats.N50, baseline.L50, stats.L50)
    assert lines[1] == 'Assembly report: sequences 3 -> %d' % len(want)
    assert lines[2] == 'Assembly report: total length 47 -> %d' % sum(lengths)
    assert lines[3] == 'Assembly report: gaps %d (of at least 2 N), gap bases %d' % (stats.gaps, stats.gap_bases)
    assert lines[4].startswith('Assembly report: bases removed by overlap merges: ')
    merged = sum(int(l.split()[1]) for l in case['expect']['merging'])
    assert int(lines[4].rsplit(' ', 1)[1]) == merged
    table = [l.rstrip('\n').split('\t') for l in open(str(on_dir / 'pass1' / 'assembly_stats.tsv'))]
    assert table[0] == ['metric', 'contigs', 'scaffolds']
    by_metric = {r[0]: r[1:] for r in table[1:]}
    assert by_metric['n'] == ['3', str(len(want))] and by_metric['N50'] == [str(baseline.N50), str(stats.N50)]
    assert by_metric['gaps'] == ['1', str(stats.gaps)] and by_metric['total'] == ['47', str(sum(lengths))]
    # the note about decide_approach: only with path extension on and N60 below the threshold
    p_note = _param(case, on_dir, assembly_report=True, extend_paths=True, ins_size_threshold=10 ** 9)
    info_note = io.StringIO()
    GO.PrintOutput(OU.case_F(case), info_note, str(on_dir), p_note, 1, unique_id=UID)
    assert 'runBESST would switch to path finding' in info_note.getvalue()
    assert 'path finding' not in info_on.getvalue()
    assert [l.split('\t') for l in open(str(on_dir / 'pass1' / 'assembly_stats.tsv'))][0] == ['metric', 'scaffolds\n']


# ---- the command line ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cli_inputs(tmp_path_factory):
    """contigs.fa (lower case, N and IUPAC in some contigs), the same with a '*' in one contig, and lib.bam"""
    from besst_amd import synth
    from tests import bam_writer
    d = tmp_path_factory.mktemp('assembly_report_cli')
    asm = synth.make_assembly(400, 1500, 7)
    batch = synth.simulate_library(asm, synth.LibrarySpec('fr', 500.0, 50.0), 30000, 8)
    rng = np.random.default_rng(9)
    seqs = {}
    for k, (n, l) in enumerate(zip(asm.names, asm.lengths)):
        s = bytearray(np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, int(l))].tobytes())
        if k % 7 == 0 and l > 400:
            s[100:130] = b'N' * 30
            s[200:260] = bytes(s[200:260]).lower()
            s[300] = ord('R')
        seqs[n] = bytes(s).decode()
    fasta, starred, bam = str(d / 'contigs.fa'), str(d / 'starred.fa'), str(d / 'lib.bam')
    star_name = list(seqs)[5]
    for path, star in ((fasta, False), (starred, True)):
        with open(path, 'w') as fh:
            for n, s in seqs.items():
                fh.write('>%s\n%s\n' % (n, s[:50] + '*' + s[51:] if star and n == star_name else s))
    bam_writer.write_bam(bam, batch)
    return dict(fasta=fasta, starred=starred, bam=bam, star_name=star_name, dir=d)


def _report_equals_fasta(report_path, fasta_bytes):
    back = seqreport.SequenceCensus.read(report_path)
    want = [(name, M.whole(seq)) for name, seq in M.split_fasta(fasta_bytes)]
    assert back.names == [n for n, _ in want]
    assert back.words.tolist() == [w for _, w in want]
    return back


@pytest.mark.parametrize('bgzf', [False, True], ids=['plain', 'bgzf_outputs'])
def test_cli_assembly_report_with_scaffolds(cli_inputs, bgzf):
    from besst_amd import cli
    out_root = cli_inputs['dir'] / ('bgzf' if bgzf else 'plain')
    argv = ['-c', cli_inputs['fasta'], '-f', cli_inputs['bam'], '-orientation', 'fr', '-o', str(out_root), '--scaffolds', '-y',
            '-max_contig_overlap', '0', '--assembly_report'] + (['--bgzf_outputs'] if bgzf else [])
    assert cli.main(argv) == 0
    out = out_root / 'BESST_output'
    with open(cli_inputs['fasta'], 'rb') as fh:
        contigs = _report_equals_fasta(str(out / 'contig_report.tsv'), fh.read())
    if bgzf:
        assert not (out / 'pass1' / 'Scaffolds-pass1.fa').exists()
        with open(str(out / 'pass1' / 'Scaffolds-pass1.fa.gz'), 'rb') as fh:
            written = gzip.decompress(fh.read())
    else:
        with open(str(out / 'pass1' / 'Scaffolds-pass1.fa'), 'rb') as fh:
            written = fh.read()
    scaffolds = _report_equals_fasta(str(out / 'pass1' / 'scaffold_report.tsv'), written)
    assert len(scaffolds) < len(contigs) and int(scaffolds.gaps.sum()) > int(contigs.gaps.sum()) > 0
    table = {r[0]: r[1:] for r in (l.rstrip('\n').split('\t') for l in open(str(out / 'pass1' / 'assembly_stats.tsv')))}
    assert table['metric'] == ['contigs', 'scaffolds']
    for census, column in ((contigs, 0), (scaffolds, 1)):
        lengths = census.length.tolist()
        assert table['n'][column] == str(len(lengths)) and table['total'][column] == str(sum(lengths))
        assert table['N50'][column] == str(M.nx(lengths, 50)) and table['L50'][column] == str(M.lx(lengths, 50))
        assert table['N90'][column] == str(M.nx(lengths, 90)) and table['gaps'][column] == str(int(census.gaps.sum()))
    stats = open(str(out / 'Statistics.txt')).read()
    assert 'Assembly report of the contigs (contig_report.tsv): %d sequences' % len(contigs) in stats
    assert 'Assembly report: N50 %s -> %s' % (table['N50'][0], table['N50'][1]) in stats
    assert 'Assembly report: sequences %d -> %d' % (len(contigs), len(scaffolds)) in stats and 'hold a byte' not in stats


def test_cli_assembly_report_without_scaffolds_names_the_odd_contig(cli_inputs, capsys):
    from besst_amd import cli
    out_root = cli_inputs['dir'] / 'contigs_only'
    assert cli.main(['-c', cli_inputs['starred'], '-f', cli_inputs['bam'], '-orientation', 'fr', '-o', str(out_root),
                     '--assembly_report', '--report_min_gap', '31']) == 0
    out = out_root / 'BESST_output'
    back = seqreport.SequenceCensus.read(str(out / 'contig_report.tsv'))
    with open(cli_inputs['starred'], 'rb') as fh:
        want = [(name, M.whole(seq, 31)) for name, seq in M.split_fasta(fh.read())]
    assert back.min_gap == 31 and back.words.tolist() == [w for _, w in want]
    assert int(back.gaps.sum()) == 0 and int(back.n_runs.sum()) > 0 and int(back.other.sum()) == 1
    assert not (out / 'pass1' / 'scaffold_report.tsv').exists() and not (out / 'pass1' / 'assembly_stats.tsv').exists()
    err = capsys.readouterr().err
    warning = [l for l in open(str(out / 'Statistics.txt')) if l.startswith('WARNING') and 'hold a byte' in l]
    assert len(warning) == 1 and cli_inputs['star_name'] in warning[0] and 'KeyError' in warning[0]
    assert warning[0].strip() in err
