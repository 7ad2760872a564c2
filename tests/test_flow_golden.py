"""A whole three-library run, pass by pass, against the reference's own run (tests/golden/flow_*.json.gz, captured by
tests/golden/make_flow_golden.py): the host hand-over from library to library.  CPU only.

  * replay: with the reference present, the fixture script gives the committed files again;
  * the package's own loop - libmetrics.get_metrics, CreateGraph.PE, cli.write_scaffolds - over all three passes with
    the device stages answered by the stand-ins of tests/fake_device.py.  The state (Contigs, Scaffolds, small_*, the
    param object) is carried by the package and never re-synchronised; every stored item of every pass must equal the
    fixture.  A failure here is a host-side defect; the kernels on the same state: tests/test_gpu_flow_golden.py.
"""
import hashlib
import importlib.util
import os
import types

import numpy as np
import pytest

from besst_amd import GenerateOutput as GO
from besst_amd import MakeScaffolds as MS
from besst_amd import session
from tests import fake_device
from tests import flow_util as FU
from tests.refharness import loader

needs_reference = pytest.mark.skipif(not loader.available(), reason='reference checkout not present')
_HERE = os.path.dirname(os.path.abspath(__file__))


def test_sequences_come_from_the_stored_seed():
    asm, libs = FU.load_inputs()
    # known answer: the first three bytes of SHA-256('abc/0') are 15d0ad, two bits per base, most significant first
    assert FU.genome_bytes('abc', 12) == b'ACCCTCAAGGTC'
    assert hashlib.sha256(FU.genome_bytes('besst', 300)).hexdigest() == \
        hashlib.sha256(FU.genome_bytes('besst', 1000)[:300]).hexdigest()
    seqs = FU.contig_sequences(asm)                              # checks a SHA-256 per contig
    assert [len(seqs[n]) for n in asm['names']] == asm['lengths']
    assert any(c.islower() for c in seqs[asm['names'][asm['edits'][0][0]]])
    assert 'N' * 31 in seqs[asm['names'][asm['edits'][1][0]]]
    assert set(''.join(seqs.values())) <= set('ACGTacgtN')       # nothing without a complement
    # a drifted generator is an error, not a new fixture
    with pytest.raises(AssertionError):
        FU.contig_sequences(dict(asm, genome_tag=asm['genome_tag'] + 'x'))
    # overlapping neighbours share their ends on the genome
    starts = FU.contig_starts(asm)
    shared = [i for i, g in enumerate(asm['gaps'][:-1]) if g < 0 and not asm['flipped'][i] and not asm['flipped'][i + 1]]
    assert len(shared) > 20
    i = shared[0]
    assert seqs[asm['names'][i]][asm['gaps'][i]:] == seqs[asm['names'][i + 1]][:-asm['gaps'][i]]
    assert 0.25 < np.mean(asm['flipped']) < 0.42 and len(libs) == 3 and int(starts[-1]) > 2_000_000


def test_flip_records_is_an_involution_and_keeps_pairs():
    asm, libs = FU.load_inputs()
    flipped = np.array(asm['flipped'], bool)
    back = FU.flip_records(libs[0], flipped)
    again = FU.flip_records(back, flipped)
    # (equal (tid, pos) rows may come back in another order: compare as sorted rows)
    def rows(b):
        m = np.stack([getattr(b, c).astype(np.int64) for c in FU.COLS], axis=1)
        return m[np.lexsort(m.T[::-1])]
    assert np.array_equal(rows(again), rows(libs[0]))
    assert not np.array_equal(back.pos, libs[0].pos)
    assert (np.diff((back.tid.astype(np.int64) << 32) | back.pos) >= 0).all()
    on = flipped[libs[0].tid]
    assert np.array_equal(np.sort(back.tid), np.sort(libs[0].tid)) and on.any()


def test_fixture_meets_its_conditions():
    """the counts the fixture script found on the reference's run (it asserts them; here: that the stored run is that one)"""
    a, b = FU.load_doc('flow_a')['conditions'], FU.load_doc('flow_b')['conditions']
    assert a['multi_contig_scaffolds'][0] >= 10 and min(a['grown_scaffolds']) >= 5
    assert a['reversed_at_positive_position'][0] >= 1 and a['clamped_junctions'][0] >= 5
    assert a['scored_edges'][1] >= 100 and a['scored_edges'][2] >= 30
    assert sum(a['merges']) >= 10 and sum(a['merges'][1:]) >= 1 and a['pass1_scaffolds_small_in_pass2'] >= 1
    assert a['contamination_ratio'][1] > 0
    for c in (a, b):
        assert c['near_ties'] == 0 and sum(c['negative_gap_edges']) >= 1
        assert min(s for s in c['smallest_relative_score_spacing'] if s is not None) >= 1e-6
        assert min(c['nearest_score_to_a_constant']) >= 1e-6
    assert b['contigs_in_graph'][0] < len(FU.load_doc('flow_assembly')['names'])


@needs_reference
def test_reference_reproduces_the_committed_fixture():
    spec = importlib.util.spec_from_file_location('make_flow_golden', os.path.join(_HERE, 'golden', 'make_flow_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh = mod.replay()
    for name in FU.SCENARIOS:
        stored, new = FU.load_doc(name), FU.roundtrip(fresh[name])
        assert set(stored) == set(new)
        for n, (p, q) in enumerate(zip(stored['passes'], new['passes'])):
            for key in p:
                assert p[key] == q[key], (name, n + 1, key)
        assert stored == new


@pytest.fixture
def stand_ins(monkeypatch):
    monkeypatch.setattr(session.device, 'GraphContext', fake_device.FakeGraphContext)
    monkeypatch.setattr(MS, 'chain_arrays', fake_device.fake_chain_arrays)
    monkeypatch.setattr(MS, 'linearize_arrays', fake_device.fake_linearize_arrays)
    monkeypatch.setattr(GO, 'PrintOutput', fake_device.fake_print_output)
    monkeypatch.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FU.UNIQUE_ID)))
    yield


@pytest.mark.parametrize('name', FU.SCENARIOS)
def test_chained_run_on_stand_ins(stand_ins, name, tmp_path):
    doc = FU.load_doc(name)
    asm, libs = FU.load_inputs()
    got = FU.run_passes(FU.package_api(), doc['scenario'], asm, libs, str(tmp_path))
    assert len(got) == len(doc['passes']) == 3
    for n, (g, w) in enumerate(zip(got, doc['passes'])):
        FU.assert_pass_equal(g, w, doc, '%s pass %d' % (name, n + 1))


class _OpenedBam(FU.RecordBatch):
    """what bamio.open_bam hands to besst_amd.cli._run, without the device: the records and a close()"""

    def close(self):
        pass


class _NoStore(object):
    """besst_amd.GenerateOutput.SequenceStore keeps the sequences in HBM; the output stand-in reads them from F"""

    def __init__(self, names, sequences, device=0):
        pass

    def close(self):
        pass


@pytest.mark.parametrize('name', FU.SCENARIOS)
def test_cli_run_on_stand_ins(stand_ins, name, monkeypatch, tmp_path):
    """besst_amd.cli itself - its own loop over the libraries, what it resets and what it carries - with the BAM front-end
    answered by the fixture's records: the three passes' files and the counting lines of Statistics.txt."""
    from besst_amd import bamio, cli
    doc = FU.load_doc(name)
    asm, libs = FU.load_inputs()
    fasta = FU.write_fasta(str(tmp_path / 'contigs.fa'), FU.contig_sequences(asm))
    opened = {'lib%d.bam' % (k + 1): _OpenedBam(b.references, b.lengths, **{c: getattr(b, c) for c in FU.COLS})
              for k, b in enumerate(libs)}
    monkeypatch.setattr(bamio, 'open_bam', lambda path, threads=None: opened[path])
    monkeypatch.setattr(GO, 'SequenceStore', _NoStore)
    argv, per_lib = FU.cli_args(doc['scenario'], fasta, sorted(opened), str(tmp_path))
    args = cli.build_parser().parse_args(argv)
    for dest, values in per_lib.items():
        setattr(args, dest, values)
    assert cli._run(args, 0) == 0
    FU.assert_files_equal_fixture(str(tmp_path / 'BESST_output'), doc, name)
