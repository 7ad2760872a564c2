"""``param.outputs_bgzf`` / ``cli --bgzf_outputs``: PrintOutput writes Scaffolds-pass<n>.fa.gz, BGZF blocks compressed on the
device (csrc/bgzf_deflate.hip) from the buffer the FASTA is produced in.  The file validates (tests/bgzf_util.py) and
decompresses to the bytes of the plain path, which tests/test_gpu_scaffold_output.py and tests/test_gpu_flow_golden.py pin
byte for byte to the reference.  Block payload and chunk size are shrunk so that the files span several chunks."""
import copy
import gzip
import io
import os
import types

import pytest

from besst_amd import GenerateOutput as GO
from tests import bgzf_util as BU
from tests import flow_util as FU
from tests import output_util as OU
from tests import text_util as TU

pytestmark = pytest.mark.gpu

DOC = OU.load_golden()
CASES = {c['name']: c for c in DOC['cases']}
UID = DOC['unique_id']
PAYLOAD = 256
CHUNK = 3 * PAYLOAD + 100                                        # -> chunks of three blocks


@pytest.fixture
def small_blocks(monkeypatch):
    monkeypatch.setattr(GO, 'BGZF_BLOCK_PAYLOAD', PAYLOAD)
    monkeypatch.setattr(GO, 'CHUNK_BYTES', CHUNK)


def read(path):
    with open(str(path), 'rb') as fh:
        return fh.read()


class Param(TU.Param):
    def __init__(self, out_dir, K, sigma, outputs_on_gpu=False, outputs_bgzf=True):
        TU.Param.__init__(self, out_dir, io.StringIO(), K, sigma, outputs_on_gpu=outputs_on_gpu)
        self.outputs_bgzf = outputs_bgzf


@pytest.mark.parametrize('name', sorted(CASES))
def test_print_output_compressed(name, small_blocks, tmp_path):
    case, want = CASES[name], CASES[name]['expect']
    param, info = Param(str(tmp_path), case['K'], case['sigma']), io.StringIO()
    F = OU.case_F(case)
    if want['key_error'] is not None:
        with pytest.raises(KeyError) as exc:
            GO.PrintOutput(F, info, str(tmp_path), param, 1, unique_id=UID)
        assert exc.value.args == (want['key_error'],)
        assert os.listdir(str(tmp_path / 'pass1')) == []          # neither .fa.gz nor .partial
    else:
        assert GO.PrintOutput(F, info, str(tmp_path), param, 1, unique_id=UID) == ()
        assert sorted(os.listdir(str(tmp_path / 'pass1'))) == ['Scaffolds-pass1.fa.gz', 'info-pass1.agp', 'info-pass1.gff']
        data = read(tmp_path / 'pass1' / 'Scaffolds-pass1.fa.gz')
        text, sizes = BU.validate(data, PAYLOAD)
        assert text == want['fasta'].encode('ascii') == gzip.decompress(data)
        assert len(sizes) == -(-len(text) // PAYLOAD)
        assert GO.last_timings['fasta_bytes'] == len(text) and GO.last_timings['fasta_file_bytes'] == len(data)
        assert GO.last_timings['bgzf_kernels'] > 0.0
        for key in ('agp', 'gff'):
            assert read(tmp_path / 'pass1' / ('info-pass1.' + key)) == want[key].encode('ascii')
        assert GO.scaffold_bytes(F, Param(None, case['K'], case['sigma']), unique_id=UID, bgzf=True, chunk_bytes=CHUNK) == data
        whole = GO.scaffold_bytes(F, Param(None, case['K'], case['sigma']), unique_id=UID, bgzf=True)
        assert BU.validate(whole, PAYLOAD)[0] == text
    assert info.getvalue() == want['information']
    assert param.information_file.getvalue().splitlines() == want['merging']


def test_the_switch_off_changes_nothing(small_blocks, tmp_path):
    case = next(c for c in DOC['cases'] if c['expect']['key_error'] is None)
    for n, param in enumerate((Param(str(tmp_path), case['K'], case['sigma'], outputs_bgzf=False),
                               TU.Param(str(tmp_path), io.StringIO(), case['K'], case['sigma'], outputs_on_gpu=False))):
        GO.PrintOutput(OU.case_F(case), io.StringIO(), str(tmp_path), param, n + 1, unique_id=UID)
        assert read(tmp_path / ('pass%d' % (n + 1)) / ('Scaffolds-pass%d.fa' % (n + 1))) == case['expect']['fasta'].encode('ascii')
        assert GO.last_timings['bgzf_kernels'] == 0.0 and GO.last_timings['fasta_file_bytes'] == GO.last_timings['fasta_bytes']


@pytest.mark.parametrize('text', ['device', 'host'])
def test_agp_and_gff_stay_as_they_are(text, small_blocks, tmp_path):
    case = max((c for c in DOC['cases'] if c['expect']['key_error'] is None), key=lambda c: len(c['expect']['fasta']))
    F = OU.case_F(case)
    if text == 'host':                                           # a float position: the layout is left to the host writer
        F = [[(n, d, float(p) if k == 0 else p, l, s) for k, (n, d, p, l, s) in enumerate(scaf)] for scaf in F]
    for n, bgzf in enumerate((False, True)):
        param = Param(str(tmp_path), case['K'], case['sigma'], outputs_on_gpu=True, outputs_bgzf=bgzf)
        GO.PrintOutput(F, io.StringIO(), str(tmp_path), param, n + 1, unique_id=UID)
        assert GO.last_timings['text'] == text
    for key in ('agp', 'gff'):
        assert read(tmp_path / 'pass1' / ('info-pass1.' + key)) == read(tmp_path / 'pass2' / ('info-pass2.' + key))
    plain = read(tmp_path / 'pass1' / 'Scaffolds-pass1.fa')
    assert len(plain) > 2 * CHUNK
    assert BU.validate(read(tmp_path / 'pass2' / 'Scaffolds-pass2.fa.gz'), PAYLOAD)[0] == plain
    assert not os.path.exists(str(tmp_path / 'pass2' / 'Scaffolds-pass2.fa'))


@pytest.mark.parametrize('n', [1, 2, 3])
@pytest.mark.parametrize('name', FU.SCENARIOS)
def test_flow_pass_compressed(name, n, monkeypatch, tmp_path):
    """a pass of the three-library runs: the same call once more with the switch on, into a directory of its own"""
    monkeypatch.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FU.UNIQUE_ID)))
    monkeypatch.setattr(GO, 'BGZF_BLOCK_PAYLOAD', 4096)
    monkeypatch.setattr(GO, 'CHUNK_BYTES', 5 * 4096 + 9)
    doc = FU.load_doc(name)
    asm, libs = FU.load_inputs()
    seqs = FU.contig_sequences(asm)
    prev = None if n == 1 else doc['passes'][n - 2]
    other = str(tmp_path / 'bgzf')
    os.mkdir(other)
    os.mkdir(str(tmp_path / 'plain'))
    real, calls = GO.PrintOutput, []

    def twice(F, Information, output_dest, param, pass_nr, store=None, unique_id=None):
        real(F, Information, output_dest, param, pass_nr, store=store, unique_id=unique_id)
        again = copy.copy(param)
        again.outputs_bgzf, again.output_directory, again.information_file = True, other, io.StringIO()
        real(F, io.StringIO(), other, again, pass_nr, store=store, unique_id=unique_id)
        calls.append(pass_nr)
    monkeypatch.setattr(GO, 'PrintOutput', twice)
    with GO.SequenceStore(list(seqs), list(seqs.values())) as store:
        FU.run_passes(FU.package_api(store), doc['scenario'], asm, libs, str(tmp_path / 'plain'), first=n - 1, last=n, prev=prev)
    assert calls == [n]
    plain = read(tmp_path / 'plain' / ('pass%d' % n) / ('Scaffolds-pass%d.fa' % n))
    data = read(tmp_path / 'bgzf' / ('pass%d' % n) / ('Scaffolds-pass%d.fa.gz' % n))
    assert len(plain) > 3 * GO.CHUNK_BYTES
    assert BU.validate(data, 4096)[0] == plain == gzip.decompress(data)
    assert len(data) < len(plain) // 2
    for key in ('agp', 'gff'):
        assert read(tmp_path / 'plain' / ('pass%d' % n) / ('info-pass%d.%s' % (n, key))) == \
            read(tmp_path / 'bgzf' / ('pass%d' % n) / ('info-pass%d.%s' % (n, key)))


# ---- through the command line ------------------------------------------------------------------------------------------------
FLAGS = ['--fasta_on_gpu', '-z', '4']


@pytest.fixture(scope='module')
def cli_runs(tmp_path_factory):
    """scenario A's inputs on disk with -z 4 (contigs are set aside as repeats), four runs: plain and --bgzf_outputs, each
    without and with --final_fasta"""
    from besst_amd import cli
    from tests import bam_writer
    asm, libs = FU.load_inputs()
    d = tmp_path_factory.mktemp('bgzf_cli')
    os.makedirs(str(d / 'in'))
    fasta = FU.write_fasta(str(d / 'in' / 'contigs.fa'), FU.contig_sequences(asm))
    bams = []
    for k, batch in enumerate(libs):
        bams.append(str(d / 'in' / ('lib%d.bam' % (k + 1))))
        bam_writer.write_bam(bams[-1], batch, block_bytes=50000 + 7000 * k, align_records=bool(k % 2))
    doc = FU.load_doc('flow_a')
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FU.UNIQUE_ID)))
        mp.setattr(GO, 'BGZF_BLOCK_PAYLOAD', 4096)
        mp.setattr(GO, 'CHUNK_BYTES', 5 * 4096 + 9)
        for key, extra in (('plain', []), ('bgzf', ['--bgzf_outputs']), ('plain_final', ['--final_fasta']),
                           ('bgzf_final', ['--final_fasta', '--bgzf_outputs'])):
            argv, per_lib = FU.cli_args(doc['scenario'], fasta, bams, str(d / key))
            assert not per_lib
            assert cli.main(argv + FLAGS + extra) == 0
            out[key] = str(d / key / 'BESST_output')
    return out


def test_cli_bgzf_outputs(cli_runs):
    for n in (1, 2, 3):
        plain = read(os.path.join(cli_runs['plain'], 'pass%d' % n, 'Scaffolds-pass%d.fa' % n))
        data = read(os.path.join(cli_runs['bgzf'], 'pass%d' % n, 'Scaffolds-pass%d.fa.gz' % n))
        assert plain.startswith(b'>scaffold_1_uid_') and BU.validate(data, 4096)[0] == plain
        assert not os.path.exists(os.path.join(cli_runs['bgzf'], 'pass%d' % n, 'Scaffolds-pass%d.fa' % n))
        for fname in ('info-pass%d.agp' % n, 'info-pass%d.gff' % n, 'edges_G.tsv'):
            assert read(os.path.join(cli_runs['bgzf'], 'pass%d' % n, fname)) == read(os.path.join(cli_runs['plain'], 'pass%d' % n, fname))
    for fname in ('repeats.fa', 'low_coverage_contigs.fa'):
        there = os.path.exists(os.path.join(cli_runs['plain'], fname))
        assert os.path.exists(os.path.join(cli_runs['bgzf'], fname)) == there
        if there:
            assert read(os.path.join(cli_runs['bgzf'], fname)) == read(os.path.join(cli_runs['plain'], fname))
    assert read(os.path.join(cli_runs['plain'], 'repeats.fa')).startswith(b'>')


def test_cli_bgzf_outputs_with_final_fasta(cli_runs):
    for n in (1, 2, 3):
        plain = read(os.path.join(cli_runs['plain_final'], 'pass%d' % n, 'Scaffolds_pass%d.fa' % n))
        scaffolds = read(os.path.join(cli_runs['plain'], 'pass%d' % n, 'Scaffolds-pass%d.fa' % n))
        assert plain.startswith(scaffolds) and len(plain) > len(scaffolds)           # (the repeats follow)
        data = read(os.path.join(cli_runs['bgzf_final'], 'pass%d' % n, 'Scaffolds_pass%d.fa.gz' % n))
        text, _sizes = BU.validate(data, None)                   # one EOF block, the file's last 28 bytes
        assert text == plain == gzip.decompress(data)
        assert sorted(f for f in os.listdir(os.path.join(cli_runs['bgzf_final'], 'pass%d' % n)) if f.startswith('Scaffolds')) == \
            ['Scaffolds_pass%d.fa.gz' % n]
    assert not os.path.exists(os.path.join(cli_runs['bgzf_final'], 'repeats.fa'))
    assert os.path.exists(os.path.join(cli_runs['plain'], 'repeats.fa'))
