"""The text of the output stage without a GPU: the plain model of tests/text_util.py against the text captured from the
reference (AGP / GFF of tests/golden/scaffold_output.json.gz and of every pass of the flow fixtures; repeats.fa /
low_coverage_contigs.fa of tests/golden/repeats_fasta.json.gz), the columns ScaffoldLayout hands to the device against that
model, the conditions under which the device text is left to the host writer, the two command-line flags, and
``cli --final_fasta`` over a three-pass run on the stand-ins of tests/fake_device.py.  The kernels themselves:
tests/test_gpu_output_text.py."""
import importlib.util
import io
import os
import types

import numpy as np
import pytest

from besst_amd import GenerateOutput as GO
from besst_amd import MakeScaffolds as MS
from besst_amd import Contig, Parameter, cli, session
from tests import fake_device
from tests import flow_util as FU
from tests import output_util as OU
from tests import text_util as TU
from tests.refharness import loader

needs_reference = pytest.mark.skipif(not loader.available(), reason='reference checkout not present')
_HERE = os.path.dirname(os.path.abspath(__file__))
DOC = OU.load_golden()
TEXT_CASES = [c for c in DOC['cases'] if c['expect']['key_error'] is None]


def test_model_equals_the_reference_on_the_output_fixture():
    assert len(TEXT_CASES) == 13
    lines = 0
    for case in TEXT_CASES:
        agp, gff, n = TU.agp_gff(OU.case_F(case), DOC['unique_id'])
        assert agp == case['expect']['agp'], case['name']
        assert gff == case['expect']['gff'], case['name']
        assert n == agp.count('\n') - 2 == gff.count('\n') - 1
        lines += agp.count('\n')
    assert lines == 1094                                         # (the two header lines of every file included)


@pytest.mark.parametrize('name', FU.SCENARIOS)
def test_model_equals_the_reference_on_the_flow_passes(name):
    doc = FU.load_doc(name)
    assert len(doc['passes']) == 3
    for n, p in enumerate(doc['passes']):
        agp, gff, lines = TU.agp_gff(TU.F_of_state(p['state']), FU.UNIQUE_ID)
        assert lines > 100
        assert agp == p['output']['agp'], (name, n + 1)
        assert gff == p['output']['gff'], (name, n + 1)


def test_short_name_rule():
    for name, want in (('a__b', 'a_'), ('_a_b', '_a'), ('_', '_'), ('abc', 'abc'), ('a_b', 'a_b'), ('a_b_c_d', 'a_b'),
                       ('__', '_'), ('', '')):
        assert TU.short_name(name) == want == '_'.join(name.split('_', 2)[:2])


def _layout(F, uid=DOC['unique_id']):
    flat = [t for scaf in OU.ordered(F) for t in scaf]
    n = len(flat)
    return GO.ScaffoldLayout(F, OU.Param(0, 0.0), uid, np.zeros(n, np.int64), np.zeros(n, np.int32)), flat


def _check_columns(F, uid=DOC['unique_id']):
    lay, flat = _layout(F, uid)
    cols = lay.text_columns()
    assert cols is not None
    assert cols['pos'].dtype == cols['len'].dtype == cols['scaffold_start'].dtype == np.int64
    assert cols['scaffold'].dtype == np.int32 and cols['gap'].dtype == bool
    assert cols['pos'].tolist() == [t[2] for t in flat] and cols['len'].tolist() == [t[3] for t in flat]
    sizes = [len(s) for s in OU.ordered(F)]
    assert cols['scaffold_start'].tolist() == [sum(sizes[:k]) for k in range(len(sizes))]
    assert cols['scaffold'].tolist() == [k for k, size in enumerate(sizes) for _ in range(size)]
    assert np.array_equal(np.flatnonzero(lay.first), cols['scaffold_start'])
    # a line per contig and a line per gap flag - in both files
    _agp, _gff, lines = TU.agp_gff(F, uid)
    assert lines == len(flat) + int(cols['gap'].sum())
    gap_lines = [int(sum(1 for l in TU.scaffold_lines(s, 'x')[0] if '\tN\t' in l)) for s in OU.ordered(F)]
    assert np.add.reduceat(cols['gap'].astype(int), cols['scaffold_start']).tolist() == gap_lines
    assert not cols['gap'][cols['scaffold_start']].any()
    return cols


def test_layout_columns_against_the_model():
    for case in TEXT_CASES:
        _check_columns(OU.case_F(case))
    for name in FU.SCENARIOS:
        for p in FU.load_doc(name)['passes']:
            _check_columns(TU.F_of_state(p['state']), FU.UNIQUE_ID)
    for n, seed in ((1, 1), (2, 2), (257, 3), (1000, 4)):
        cols = _check_columns(TU.seeded_F(n, seed)[0])
    assert cols['gap'].any() and (cols['pos'] < 0).any() and (cols['len'] == 0).any()
    cols = _check_columns(TU.seeded_F(120, 5, coords=True)[0])
    assert int(cols['pos'].max()) == 2 ** 62 - 1
    # numpy integers are integers
    F = [[('a', True, np.int64(5), np.int32(7), ''), ('b', False, np.int64(20), np.int32(1), '')]]
    assert _check_columns(F)['gap'].tolist() == [False, True]
    assert _check_columns([])['pos'].shape == (0,)


def test_what_is_left_to_the_host_writer():
    ok = [[('a', True, 0, 10, ''), ('b', False, 15, 3, '')]]
    assert _layout(ok)[0].text_columns() is not None
    for bad in (12.0, 2 ** 62, -2 ** 62, np.float32(3)):
        for slot in (2, 3):
            t = list(ok[0][1])
            t[slot] = bad
            F = [[ok[0][0], tuple(t)]]
            assert _layout(F)[0].text_columns() is None, (bad, slot)
    for edge in (2 ** 62 - 1, -(2 ** 62) + 1):
        assert _layout([[('a', True, edge, 0, '')]])[0].text_columns() is not None
    for uid in (1.5, '17', None, 2 ** 63, True):
        assert _layout(ok, uid)[0].text_columns() is None, uid
    for uid in (0, 10 ** 12, np.int64(7), -3):
        assert _layout(ok, uid)[0].text_columns() is not None, uid
    # a name that is not ASCII: the store cannot build its pool, the emitter declines
    store = GO.SequenceStore.__new__(GO.SequenceStore)
    store._name_list = ['ok', 'café']
    with pytest.raises(UnicodeEncodeError):
        store.name_pool()
    em = types.SimpleNamespace(layout=_layout(ok)[0], store=store)
    assert GO._TextEmitter.make(em) is None
    # and a layout the device cannot take is declined before the store is asked
    em = types.SimpleNamespace(layout=_layout([[('a', True, 0.5, 1, '')]])[0], store=None)
    assert GO._TextEmitter.make(em) is None


def test_switches_default_to_off():
    assert Parameter.parameter().outputs_on_gpu is False
    assert GO.SequenceStore.batch_fasta is False
    args = cli.build_parser().parse_args(['-c', 'c.fa', '-f', 'a.bam', '-orientation', 'fr'])
    assert args.outputs_on_gpu is False and args.final_fasta is False
    args = cli.build_parser().parse_args(['-c', 'c.fa', '-f', 'a.bam', '-orientation', 'fr', '--outputs_on_gpu',
                                          '--final_fasta', '--scaffolds', '-y'])
    assert args.outputs_on_gpu is True and args.final_fasta is True
    # the exported units of the kernels are the header's
    text = open(os.path.join(os.path.dirname(_HERE), 'include', 'besst_amd.h')).read()
    for macro, value in (('BESST_TEXT_THREADS', GO.TEXT_THREADS), ('BESST_TEXT_SCAN_CHUNK', GO.TEXT_SCAN_CHUNK),
                         ('BESST_TEXT_TILE_BYTES', GO.TEXT_TILE_BYTES), ('BESST_WRAP_TILE_BYTES', GO.WRAP_TILE_BYTES),
                         ('BESST_TEXT_INFO_WORDS', GO.TEXT_INFO_WORDS), ('BESST_TEXT_AGP', GO.TEXT_AGP),
                         ('BESST_TEXT_GFF', GO.TEXT_GFF)):
        assert '#define %s %d\n' % (macro, value) in text, macro


def test_final_fasta_needs_scaffolds():
    with pytest.raises(SystemExit) as exc:
        cli.main(['-c', 'c.fa', '-f', 'a.bam', '-orientation', 'fr', '--final_fasta'])
    assert '--final_fasta needs --scaffolds' in str(exc.value)


# ---- repeats.fa / low_coverage_contigs.fa -------------------------------------------------------------------------------
def test_wrapped_fasta_model_equals_the_reference():
    doc = TU.load_repeats_golden()
    lengths = sorted(len(c[1]) for c in doc['contigs'])
    assert {0, 1, 59, 60, 61, 120, 121} <= set(lengths) and len(lengths) >= 12
    for key in ('repeats', 'low_coverage'):
        rows = doc['orders'][key]
        assert TU.wrapped_fasta([doc['contigs'][i][:2] for i in rows]) == doc['expect'][key], key
    assert doc['expect']['repeats'].count('\n') == sum(1 + (len(doc['contigs'][i][1]) + 59) // 60
                                                       for i in doc['orders']['repeats'])


def test_host_writers_equal_the_reference(tmp_path):
    """the package's loops (what runs without batch_fasta): same files, same dict deletions"""
    doc = TU.load_repeats_golden()
    objs, dicts = [], dict(Contigs={}, small_contigs={})
    for name, seq, where in doc['contigs']:
        c = Contig.contig(name)
        c.sequence, c.length = seq, len(seq)
        objs.append(c)
        dicts[where][name] = c
    GO.PrintOutRepeats([objs[i] for i in doc['orders']['repeats']], dicts['Contigs'], str(tmp_path), dicts['small_contigs'])
    GO.PrintOut_low_cowerage_contigs([objs[i] for i in doc['orders']['low_coverage']], dicts['Contigs'], str(tmp_path),
                                     dicts['small_contigs'])
    for key, fname in (('repeats', 'repeats.fa'), ('low_coverage', 'low_coverage_contigs.fa')):
        with open(str(tmp_path / fname), newline='') as fh:
            assert fh.read() == doc['expect'][key]
    assert {k: list(v) for k, v in dicts.items()} == doc['expect']['left']


@needs_reference
def test_reference_reproduces_the_repeats_fixture():
    spec = importlib.util.spec_from_file_location('make_repeats_golden', os.path.join(_HERE, 'golden', 'make_repeats_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert FU.roundtrip(mod.build()) == TU.load_repeats_golden()


# ---- cli --final_fasta on the stand-ins ------------------------------------------------------------------------------------
class _OpenedBam(FU.RecordBatch):
    def close(self):
        pass


class _NoStore(object):
    batch_fasta = False

    def __init__(self, names, sequences, device=0):
        pass

    def close(self):
        pass


def _run_on_stand_ins(monkeypatch, tmp_path, name, extra, seen=None):
    doc = FU.load_doc(name)
    asm, libs = FU.load_inputs()
    out = tmp_path / 'BESST_output'

    def print_output(F, Information, output_dest, param, pass_nr, store=None, unique_id=None):
        fake_device.fake_print_output(F, Information, output_dest, param, pass_nr, store=store, unique_id=unique_id)
        if seen is not None:
            with open(str(out / ('pass%d' % pass_nr) / ('Scaffolds-pass%d.fa' % pass_nr)), 'rb') as fa, \
                    open(str(out / 'repeats.fa'), 'rb') as rep:
                seen.append((fa.read(), rep.read()))

    monkeypatch.setattr(session.device, 'GraphContext', fake_device.FakeGraphContext)
    monkeypatch.setattr(MS, 'chain_arrays', fake_device.fake_chain_arrays)
    monkeypatch.setattr(MS, 'linearize_arrays', fake_device.fake_linearize_arrays)
    monkeypatch.setattr(GO, 'PrintOutput', print_output)
    monkeypatch.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FU.UNIQUE_ID)))
    monkeypatch.setattr(GO, 'SequenceStore', _NoStore)
    from besst_amd import bamio
    fasta = FU.write_fasta(str(tmp_path / 'contigs.fa'), FU.contig_sequences(asm))
    opened = {'lib%d.bam' % (k + 1): _OpenedBam(b.references, b.lengths, **{c: getattr(b, c) for c in FU.COLS})
              for k, b in enumerate(libs)}
    monkeypatch.setattr(bamio, 'open_bam', lambda path, threads=None: opened[path])
    argv, per_lib = FU.cli_args(doc['scenario'], fasta, sorted(opened), str(tmp_path))
    args = cli.build_parser().parse_args(argv + extra)
    for dest, values in per_lib.items():
        setattr(args, dest, values)
    assert cli._run(args, 0) == 0
    return out, doc


def test_cli_final_fasta_on_stand_ins(monkeypatch, tmp_path):
    seen = []
    out, doc = _run_on_stand_ins(monkeypatch, tmp_path, 'flow_b', ['--final_fasta'], seen)
    assert len(seen) == 3 and all(rep.startswith(b'>') for _fa, rep in seen)     # (-z 4: contigs are set aside as repeats)
    for n, (scaffolds, repeats) in enumerate(seen):
        pass_dir = out / ('pass%d' % (n + 1))
        with open(str(pass_dir / ('Scaffolds_pass%d.fa' % (n + 1))), 'rb') as fh:
            assert fh.read() == scaffolds + repeats, n + 1
        assert not (pass_dir / ('Scaffolds-pass%d.fa' % (n + 1))).exists()
        # the scaffold part is the reference's file
        want = doc['passes'][n]['output']['fasta']
        got = FU.fasta_summary(scaffolds.decode('ascii'))
        assert got['headers'] == want['headers'] and got['sha256'] == want['sha256']
        for key in ('agp', 'gff'):
            with open(str(pass_dir / ('info-pass%d.%s' % (n + 1, key))), newline='') as fh:
                assert fh.read() == doc['passes'][n]['output'][key]
    assert not (out / 'repeats.fa').exists()


def test_cli_without_final_fasta_leaves_the_files_as_before(monkeypatch, tmp_path):
    out, doc = _run_on_stand_ins(monkeypatch, tmp_path, 'flow_a', [])
    FU.assert_files_equal_fixture(str(out), doc, 'flow_a')
    assert (out / 'repeats.fa').exists()
    assert not any((out / ('pass%d' % n) / ('Scaffolds_pass%d.fa' % n)).exists() for n in (1, 2, 3))
