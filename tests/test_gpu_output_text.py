"""The text of the output stage on the device (csrc/emit_text.hip behind besst_amd.GenerateOutput): AGP and GFF with
``param.outputs_on_gpu``, repeats.fa / low_coverage_contigs.fa with ``SequenceStore.batch_fasta``, and the final files of
``cli --final_fasta``.  Byte for byte against the text captured from the reference where a fixture holds it, else against
GenerateOutput._write_agp_gff / _write_fasta (the host writers, pinned to the reference by tests/test_scaffold_output.py
and tests/test_output_text.py) - never against the device path itself."""
import io
import os
import re
import socket
import subprocess
import sys
import types

import numpy as np
import pytest

from besst_amd import Contig
from besst_amd import GenerateOutput as GO
from tests import flow_util as FU
from tests import output_util as OU
from tests import text_util as TU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = OU.load_golden()
CASES = {c['name']: c for c in DOC['cases'] if c['expect']['key_error'] is None}
UID = DOC['unique_id']
UNITS = (GO.TEXT_THREADS, GO.TEXT_SCAN_CHUNK, GO.TEXT_TILE_BYTES, GO.WRAP_TILE_BYTES)


def host_text(F, uid):
    """(AGP, GFF) bytes from the host writer"""
    n = sum(len(s) for s in F)
    lay = GO.ScaffoldLayout(F, OU.Param(0, 0.0), uid, np.zeros(n, np.int64), np.zeros(n, np.int32))
    agp, gff = io.StringIO(), io.StringIO()
    GO._write_agp_gff(lay, agp, gff)
    return agp.getvalue().encode('ascii'), gff.getvalue().encode('ascii')


def device_text(F, uid, ranges=None):
    got = GO.text_bytes(F, TU.Param(), unique_id=uid, ranges=ranges)
    assert got is not None, 'the layout was left to the host writer'
    return got


def assert_same(got, want, what):
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError('%s: %d / %d bytes, first difference at byte %d: %r != %r' % (
            what, len(got), len(want), at, got[max(0, at - 60):at + 20], want[max(0, at - 60):at + 20]))


# ---- the fixtures captured from the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_print_output_on_the_device_equals_the_reference(name, tmp_path):
    case, want = CASES[name], CASES[name]['expect']
    param = TU.Param(str(tmp_path), io.StringIO(), case['K'], case['sigma'])
    info = io.StringIO()
    assert GO.PrintOutput(OU.case_F(case), info, str(tmp_path), param, 1, unique_id=UID) == ()
    assert GO.last_timings['text'] == 'device' and GO.last_timings['text_bytes'] == len(want['agp']) + len(want['gff'])
    for key, fname in (('fasta', 'Scaffolds-pass1.fa'), ('agp', 'info-pass1.agp'), ('gff', 'info-pass1.gff')):
        with open(str(tmp_path / 'pass1' / fname), 'rb') as fh:
            assert_same(fh.read(), want[key].encode('ascii'), key)
    assert sorted(os.listdir(str(tmp_path / 'pass1'))) == ['Scaffolds-pass1.fa', 'info-pass1.agp', 'info-pass1.gff']
    assert info.getvalue() == want['information']
    assert param.information_file.getvalue().splitlines() == want['merging']


@pytest.mark.parametrize('n', [1, 2, 3])
@pytest.mark.parametrize('name', FU.SCENARIOS)
def test_flow_pass_on_the_device_equals_the_reference(name, n, monkeypatch, tmp_path):
    """a pass of the three-library runs from the state the reference left, the run's store serving the names"""
    monkeypatch.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FU.UNIQUE_ID)))
    doc = FU.load_doc(name)
    asm, libs = FU.load_inputs()
    seqs = FU.contig_sequences(asm)
    prev = None if n == 1 else doc['passes'][n - 2]
    texts = []
    with GO.SequenceStore(list(seqs), list(seqs.values())) as store:
        api = FU.package_api(store)
        inner = api.algorithm_and_output

        def with_the_switch(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, Information, param, pass_nr):
            param.outputs_on_gpu = True
            inner(G, G_prime, Contigs, small_contigs, Scaffolds, small_scaffolds, Information, param, pass_nr)
            texts.append(GO.last_timings.get('text'))
        api.algorithm_and_output = with_the_switch
        got = FU.run_passes(api, doc['scenario'], asm, libs, str(tmp_path), first=n - 1, last=n, prev=prev)
    assert texts == ['device']
    FU.assert_pass_equal(got[0], doc['passes'][n - 1], doc, '%s pass %d' % (name, n), device=True)


# ---- seeded layouts ----------------------------------------------------------------------------------------------------------
def _counts():
    out = {1, 2, 63, 64, 65, 255, 256, 257, 4097}
    for u in UNITS:
        out |= {u - 1, u, u + 1}
    return sorted(out)


@pytest.mark.parametrize('n', _counts())
def test_seeded_layouts(n):
    """contig counts on and next to every unit of the kernels; scaffolds of 1-6 contigs, gaps -1 / 0 / 1 and wider,
    lengths 0 and 1, negative starts, names of 1-300 bytes with every underscore pattern"""
    F, names = TU.seeded_F(n, 100 + n)
    agp, gff = device_text(F, 1700000000)
    want = host_text(F, 1700000000)
    assert_same(agp, want[0], 'AGP')
    assert_same(gff, want[1], 'GFF')
    assert agp.count(b'\n') >= n + 2
    if n > 60:
        offsets = np.cumsum([len(x) for x in names])
        assert (offsets % 2).any() and not (offsets % 2).all()    # names at odd and even pool offsets
        assert b'\tN\t1\t' in agp and b'\t1\t0\t' in agp and b'\t-' in agp


@pytest.mark.parametrize('n', [257, 4097, GO.TEXT_TILE_BYTES + 1])
def test_scaffold_boundaries_on_the_units(n):
    """a scaffold starts on and next to every unit below n (and the last scaffold has one contig)"""
    edges = sorted({e + d for e in (64, 256, 1024, 4096, GO.TEXT_TILE_BYTES) for d in (-1, 0, 1) if 0 < e + d < n} | {n - 1})
    F, _ = TU.seeded_F(n, 7, boundaries=edges)
    assert len(F) == len(edges) + 1
    got, want = device_text(F, 0), host_text(F, 0)
    assert_same(got[0], want[0], 'AGP')
    assert_same(got[1], want[1], 'GFF')


def test_component_counter_and_scaffold_ordinal():
    # one scaffold of 600 contigs with a gap at every junction: components 1..1199
    scaf = [('c_%d' % i, i % 3 == 0, 50 * i, 49, '') for i in range(600)]
    got, want = device_text([scaf], 1), host_text([scaf], 1)
    assert_same(got[0], want[0], 'AGP')
    assert_same(got[1], want[1], 'GFF')
    comps = [int(l.split(b'\t')[3]) for l in got[0].splitlines()[2:]]
    assert comps == list(range(1, 1200))
    # 100 001 one-contig scaffolds: the ordinal crosses every power of ten up to 10^5
    n = 100001
    F = [[('s%d' % i, True, 0, 7, '')] for i in range(n)]
    got, want = device_text(F, 10 ** 12), host_text(F, 10 ** 12)
    assert_same(got[0], want[0], 'AGP')
    assert_same(got[1], want[1], 'GFF')
    assert got[0].endswith(b'scaffold_100001_uid_1000000000000\t1\t7\t1\tW\ts0\t1\t7\t+\n')


@pytest.mark.parametrize('uid', [0, 1700000000, 10 ** 12])
def test_coordinates_across_the_digit_boundaries(uid):
    F, _ = TU.seeded_F(400, 31, coords=True)
    got, want = device_text(F, uid), host_text(F, uid)
    assert_same(got[0], want[0], 'AGP')
    assert_same(got[1], want[1], 'GFF')
    for value in (9, 10, 99, 100, 10 ** 9, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 10 ** 12, 2 ** 62 - 1, -1, -30, -10 ** 5):
        assert b'\t%d\t' % value in got[0], value
    assert b'_uid_%d\t' % uid in got[1]


def test_ranges_of_the_files():
    F, names = TU.seeded_F(1500, 77)
    want = host_text(F, UID)
    for which, whole in enumerate(want):
        total = len(whole)
        assert total > 4 * GO.TEXT_TILE_BYTES
        inside_number = whole.index(b'_uid_17000') + 8
        inside_name = whole.index(b'y' * 300) + 150
        line_end = whole.index(b'\n', total // 2) + 1
        ranges = [(0, total), (1, total - 1), (total // 3, total // 3), (0, inside_number), (17, inside_name), (5, line_end),
                  (line_end, total), (GO.TEXT_TILE_BYTES - 1, GO.TEXT_TILE_BYTES + 1), (total - 1, total)]
        step = 4096 + 1
        chunks = [(b, min(total, b + step)) for b in range(0, total, step)]
        got = device_text(F, UID, ranges + chunks)[which]
        for (b, e), part in zip(ranges, got):
            assert_same(part, whole[b:e], 'file %d, range %d..%d' % (which, b, e))
        assert_same(b''.join(got[len(ranges):]), whole, 'file %d in chunks of %d' % (which, step))


def test_store_names_by_row(tmp_path):
    """a run's store: rows are looked up by name, the names come from its pool (odd offsets, rows out of order)"""
    names = TU.seeded_names(300, 9)
    rng = np.random.default_rng(9)
    seqs = [''.join('ACGT'[int(x)] for x in rng.integers(0, 4, int(rng.integers(1, 40)))) for _ in names]
    order = rng.permutation(300)
    F, pos = [], 0
    for k in range(0, 300, 3):
        scaf = []
        for i in order[k:k + 3]:
            scaf.append((names[i], bool(i % 2), pos, len(seqs[i]), seqs[i]))
            pos += len(seqs[i]) + int(rng.integers(-2, 30))
        F.append(scaf)
    with GO.SequenceStore(names, seqs) as store:
        for switch in (False, True):
            param = TU.Param(str(tmp_path), io.StringIO(), 0, 10.0, outputs_on_gpu=switch)
            GO.PrintOutput(F, io.StringIO(), str(tmp_path), param, 1 + switch, store=store, unique_id=UID)
            assert GO.last_timings.get('text') == ('device' if switch else None)
    for fname in ('Scaffolds-pass%d.fa', 'info-pass%d.agp', 'info-pass%d.gff'):
        with open(str(tmp_path / 'pass1' / (fname % 1)), 'rb') as a, open(str(tmp_path / 'pass2' / (fname % 2)), 'rb') as b:
            assert_same(b.read(), a.read(), fname)


def test_a_float_position_is_left_to_the_host(tmp_path):
    F = [[('a_1', True, 0, 10, 'ACGTACGTAC'), ('b_2', False, 12.0, 4, 'ACGT')]]
    param = TU.Param(str(tmp_path), io.StringIO(), 0, 1.0)
    GO.PrintOutput(F, io.StringIO(), str(tmp_path), param, 1, unique_id=UID)
    assert GO.last_timings['text'] == 'host'
    want = host_text(F, UID)
    for key, text in zip(('agp', 'gff'), want):
        with open(str(tmp_path / 'pass1' / ('info-pass1.' + key)), 'rb') as fh:
            assert fh.read() == text
    assert b'\t12.0\t' in want[0]                                # (what str() makes of it, which the device does not)
    assert GO.text_bytes(F, param, unique_id=UID) is None


# ---- wrapped FASTA -----------------------------------------------------------------------------------------------------------
WRAP_LENGTHS = [0, 1, 59, 60, 61, 119, 120, 121, GO.WRAP_TILE_BYTES - 1, GO.WRAP_TILE_BYTES, GO.WRAP_TILE_BYTES + 1, 7, 600,
                (1 << 20) + 7, 0, 61]


@pytest.fixture(scope='module')
def wrap_store():
    rng = np.random.default_rng(41)
    alphabet = np.frombuffer(b'ACGTNacgtnRYKM', dtype=np.uint8)
    names = TU.seeded_names(len(WRAP_LENGTHS), 4)
    seqs = [alphabet[rng.integers(0, len(alphabet), n)].tobytes().decode('ascii') for n in WRAP_LENGTHS]
    with GO.SequenceStore(names, seqs) as store:
        yield store, names, seqs


def host_fasta(names, seqs, rows):
    out = io.StringIO()
    for r in rows:
        GO._write_fasta(out, names[r], seqs[r])
    return out.getvalue().encode('ascii')


def test_wrapped_fasta_of_every_length(wrap_store):
    store, names, seqs = wrap_store
    for rows in ([r] for r in range(len(seqs))):
        assert_same(GO.wrapped_fasta_bytes(store, rows), host_fasta(names, seqs, rows), 'row %d' % rows[0])
    assert GO.wrapped_fasta_bytes(store, []) == b''
    with pytest.raises(ValueError):
        GO.wrapped_fasta_bytes(store, [len(seqs)])


def test_wrapped_fasta_rows_out_of_order_and_repeated(wrap_store):
    store, names, seqs = wrap_store
    rows = [5, 0, 13, 1, 1, 8, 9, 10, 0, 14, 2, 3, 4, 15, 6, 7, 11, 12, 5]
    whole = host_fasta(names, seqs, rows)
    assert_same(GO.wrapped_fasta_bytes(store, rows), whole, 'all rows')
    total = len(whole)
    inside_name = whole.index(b'y' * 300) + 100
    line_end = whole.index(b'\n', total // 2) + 1
    ranges = [(0, total), (1, total - 1), (9, 9), (3, inside_name), (7, line_end), (line_end - 1, total),
              (GO.WRAP_TILE_BYTES - 7, GO.WRAP_TILE_BYTES + 9), (total - 1, total)]
    step = 4096 + 1
    chunks = [(b, min(total, b + step)) for b in range(0, total, step)]
    got = GO.wrapped_fasta_bytes(store, rows, ranges + chunks)
    for (b, e), part in zip(ranges, got):
        assert_same(part, whole[b:e], 'range %d..%d' % (b, e))
    assert_same(b''.join(got[len(ranges):]), whole, 'chunks of %d' % step)


def test_wrapped_fasta_equals_the_reference(tmp_path):
    doc = TU.load_repeats_golden()
    names, seqs = [c[0] for c in doc['contigs']], [c[1] for c in doc['contigs']]
    with GO.SequenceStore(names, seqs) as store:
        for key in ('repeats', 'low_coverage'):
            assert_same(GO.wrapped_fasta_bytes(store, doc['orders'][key]), doc['expect'][key].encode('ascii'), key)


@pytest.mark.parametrize('batch', [False, True])
def test_repeat_writers_from_the_store(batch, monkeypatch, tmp_path):
    """PrintOutRepeats / PrintOut_low_cowerage_contigs on SequenceRefs: the reference's files and deletions either way;
    with batch_fasta not one contig is fetched"""
    doc = TU.load_repeats_golden()
    fetched = []
    real = GO.SequenceStore.fetch
    monkeypatch.setattr(GO.SequenceStore, 'fetch', lambda self, row: fetched.append(row) or real(self, row))
    with GO.SequenceStore([c[0] for c in doc['contigs']], [c[1] for c in doc['contigs']]) as store:
        store.batch_fasta = batch
        refs = store.contig_dict()
        objs, dicts = [], dict(Contigs={}, small_contigs={})
        for name, seq, where in doc['contigs']:
            c = Contig.contig(name)
            c.sequence, c.length = refs[name], len(seq)
            objs.append(c)
            dicts[where][name] = c
        GO.PrintOutRepeats([objs[i] for i in doc['orders']['repeats']], dicts['Contigs'], str(tmp_path), dicts['small_contigs'])
        GO.PrintOut_low_cowerage_contigs([objs[i] for i in doc['orders']['low_coverage']], dicts['Contigs'], str(tmp_path),
                                         dicts['small_contigs'])
    for key, fname in (('repeats', 'repeats.fa'), ('low_coverage', 'low_coverage_contigs.fa')):
        with open(str(tmp_path / fname), 'rb') as fh:
            assert_same(fh.read(), doc['expect'][key].encode('ascii'), key)
    assert {k: list(v) for k, v in dicts.items()} == doc['expect']['left']
    if batch:
        assert fetched == []
    else:
        assert sorted(fetched) == sorted(i for key in ('repeats', 'low_coverage') for i in doc['orders'][key]
                                         if doc['contigs'][i][1])       # (an empty sequence is never asked for)


# ---- through the command line ------------------------------------------------------------------------------------------------
def _tree(out, uid=False):
    """{relative path: bytes} of an output directory, without Statistics.txt (it holds wall times)"""
    files = {}
    for base, _dirs, names in os.walk(out):
        for name in names:
            if name == 'Statistics.txt':
                continue
            with open(os.path.join(base, name), 'rb') as fh:
                data = fh.read()
            if uid:                                              # (another process's clock)
                data = re.sub(br'_uid_\d+', b'_uid_%d' % FU.UNIQUE_ID, data)
            files[os.path.relpath(os.path.join(base, name), out)] = data
    return files


FLAGS = ['--fasta_on_gpu', '--final_fasta', '-z', '4']


@pytest.fixture(scope='module')
def cli_runs(tmp_path_factory):
    """scenario A's inputs on disk with -z 4 (contigs are set aside as repeats): the command without --outputs_on_gpu, and
    with it - there every PrintOutput is followed by a look at the two files the final file is made of"""
    from besst_amd import cli
    from tests import bam_writer
    asm, libs = FU.load_inputs()
    d = tmp_path_factory.mktemp('text_cli')
    fasta = FU.write_fasta(str(d / 'contigs.fa'), FU.contig_sequences(asm))
    bams = []
    for k, batch in enumerate(libs):
        bams.append(str(d / ('lib%d.bam' % (k + 1))))
        bam_writer.write_bam(bams[-1], batch, block_bytes=50000 + 7000 * k, align_records=bool(k % 2))
    doc = FU.load_doc('flow_a')
    seen, texts = [], []
    real = GO.PrintOutput

    def watched(F, Information, output_dest, param, pass_nr, store=None, unique_id=None):
        real(F, Information, output_dest, param, pass_nr, store=store, unique_id=unique_id)
        texts.append(GO.last_timings.get('text'))
        with open(os.path.join(output_dest, 'pass%d' % pass_nr, 'Scaffolds-pass%d.fa' % pass_nr), 'rb') as fa, \
                open(os.path.join(output_dest, 'repeats.fa'), 'rb') as rep:
            seen.append((fa.read(), rep.read()))

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FU.UNIQUE_ID)))
        argv, per_lib = FU.cli_args(doc['scenario'], fasta, bams, str(d / 'host'))
        assert not per_lib
        assert cli.main(argv + FLAGS) == 0
        mp.setattr(GO, 'PrintOutput', watched)
        argv, _ = FU.cli_args(doc['scenario'], fasta, bams, str(d / 'device'))
        assert cli.main(argv + FLAGS + ['--outputs_on_gpu']) == 0
    return dict(fasta=fasta, bams=bams, doc=doc, host=str(d / 'host' / 'BESST_output'),
                device=str(d / 'device' / 'BESST_output'), seen=seen, texts=texts)


def test_cli_outputs_on_gpu_leaves_the_same_files(cli_runs):
    host, device = _tree(cli_runs['host']), _tree(cli_runs['device'])
    assert sorted(host) == sorted(device)
    for path in sorted(host):
        assert_same(device[path], host[path], path)
    assert cli_runs['texts'] == ['device'] * 3 and any(rep.startswith(b'>') for _fa, rep in cli_runs['seen'])
    assert 'repeats.fa' not in device
    for n, (scaffolds, repeats) in enumerate(cli_runs['seen']):
        assert scaffolds.startswith(b'>scaffold_1_uid_')
        assert_same(device[os.path.join('pass%d' % (n + 1), 'Scaffolds_pass%d.fa' % (n + 1))], scaffolds + repeats,
                    'the final file of pass %d' % (n + 1))
        assert os.path.join('pass%d' % (n + 1), 'Scaffolds-pass%d.fa' % (n + 1)) not in device


def test_cli_outputs_on_gpu_under_two_ranks(cli_runs, tmp_path):
    """two gloo ranks on one GPU: rank 0 writes the files of the one-process run"""
    argv, _ = FU.cli_args(cli_runs['doc']['scenario'], cli_runs['fasta'], cli_runs['bams'], str(tmp_path))
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, BESST_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), '-m', 'besst_amd.cli'] + argv + FLAGS + ['--outputs_on_gpu']
    done = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert done.returncode == 0, done.stdout.decode()[-3000:]
    host, ranks = _tree(cli_runs['host'], uid=True), _tree(str(tmp_path / 'BESST_output'), uid=True)
    assert sorted(host) == sorted(ranks)
    for path in sorted(host):
        assert_same(ranks[path], host[path], path)
