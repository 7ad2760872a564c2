"""The kernels on the state a real multi-library run leaves: every pass of the two three-library scenarios of
tests/golden/flow_*.json.gz (the reference's own run, see tests/golden/make_flow_golden.py) on the device.

  * per pass, from the fixture's state before it (resynchronised), for both forms of the record loop: metrics, graphs,
    dicts, state after step 5, AGP / GFF text and FASTA digests - a failure names scenario, pass and stage;
  * the record loop alone on the contig table the reference built (reversed contigs at positions above 0, clamped
    junctions, scaffolds below the next library's threshold) against oracle.py_oracle.record_loop;
  * chained through besst_amd.cli (FASTA and three BAM files on disk), one process and two gloo ranks on one GPU: the
    three passes' files equal the reference's.
The host hand-over alone, without a GPU: tests/test_flow_golden.py.
"""
import os
import subprocess
import sys
import types

import pytest

from besst_amd import GenerateOutput as GO
from oracle import py_oracle as O
from tests import flow_util as FU
from tests import gpu_util as DU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def fixed_uid(monkeypatch):
    """the uid in the scaffold names is the clock (GenerateOutput.py:209): GenerateOutput's own view of it is pinned"""
    monkeypatch.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FU.UNIQUE_ID)))


@pytest.mark.parametrize('path', ['0', '1'])
@pytest.mark.parametrize('n', [1, 2, 3])
@pytest.mark.parametrize('name', FU.SCENARIOS)
def test_pass_from_the_state_the_reference_left(name, n, path, fixed_uid, monkeypatch, tmp_path):
    monkeypatch.setenv('BESST_RECORD_PATH', path)
    doc = FU.load_doc(name)
    asm, libs = FU.load_inputs()
    seqs = FU.contig_sequences(asm)
    prev = None if n == 1 else doc['passes'][n - 2]
    with GO.SequenceStore(list(seqs), list(seqs.values())) as store:
        got = FU.run_passes(FU.package_api(store), doc['scenario'], asm, libs, str(tmp_path), first=n - 1, last=n,
                            prev=prev)
    FU.assert_pass_equal(got[0], doc['passes'][n - 1], doc, '%s pass %d (record path %s)' % (name, n, path), device=True)


def contig_table_before(doc, asm, n):
    """The per-tid table of pass n (n >= 2) from the fixture alone: placements and scaffold lengths as pass n - 1 left
    them; a scaffold of `Scaffolds` shorter than the library's contig_threshold counts as small (CleanObjects,
    CreateGraph.py:797-807), a small one stays small."""
    prev, thr = doc['passes'][n - 2]['state'], doc['passes'][n - 1]['metrics']['contig_threshold']
    s_length = {key: length for key, _, _, length in prev['scaffolds'] + prev['small_scaffolds']}
    tid = {name: i for i, name in enumerate(asm['names'])}
    nc = len(tid)
    tab = dict(cls=[0] * nc, scaf=[0] * nc, slen=[0] * nc, cpos=[0] * nc, clen=[0] * nc, cdir=[True] * nc)
    for group, large in ((prev['contigs'], True), (prev['small_contigs'], False)):
        for name, scaf, pos, direction, length, _cov in group:
            i = tid[name]
            tab['cls'][i] = 1 if large and s_length[scaf] >= thr else 2
            tab['scaf'][i], tab['slen'][i] = scaf, s_length[scaf]
            tab['cpos'][i], tab['clen'][i], tab['cdir'][i] = pos, length, direction
    return tab


@pytest.mark.parametrize('path', ['0', '1'])
@pytest.mark.parametrize('n', [2, 3])
@pytest.mark.parametrize('name', FU.SCENARIOS)
def test_record_loop_on_the_captured_contig_table(name, n, path, monkeypatch):
    monkeypatch.setenv('BESST_RECORD_PATH', path)
    doc = FU.load_doc(name)
    asm, libs = FU.load_inputs()
    tab = contig_table_before(doc, asm, n)
    # the table is what the issue is about: reversed contigs at positions above 0 inside multi-contig scaffolds, both classes
    assert sum(1 for d, p in zip(tab['cdir'], tab['cpos']) if not d and p > 0) >= 50
    assert {1, 2} <= set(tab['cls']) and any(s > c for s, c in zip(tab['slen'], tab['clen']))
    m, lib = doc['passes'][n - 1]['metrics'], doc['scenario']['libraries'][n - 1]
    p = O.LibParams(read_len=m['read_len'], ins_size_threshold=m['ins_size_threshold'], min_mapq=11,
                    orientation=lib['orientation'], detect_duplicate=doc['scenario']['detect_duplicate'],
                    extend_paths=False, no_score=False)
    batch = libs[n - 1]
    want = O.record_loop({c: getattr(batch, c).tolist() for c in FU.COLS}, tab, p)
    # (the fixture script asserts 100 / 30 scored edges in passes 2 / 3; every scored edge is a link row of this table)
    assert want.count > 1000 and sum(1 for r in want.edges.values() if r.n) >= (100 if n == 2 else 30)
    table, aligned, ctr = DU.device_build(batch, tab, p)
    DU.assert_matches_oracle(table, aligned, ctr, want, len(batch.references))


# ---- through the command line --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """contigs.fa and lib1..3.bam of the fixture's inputs, written once"""
    from tests import bam_writer
    asm, libs = FU.load_inputs()
    d = tmp_path_factory.mktemp('flow_inputs')
    fasta = FU.write_fasta(str(d / 'contigs.fa'), FU.contig_sequences(asm))
    bams = []
    for k, batch in enumerate(libs):
        bams.append(str(d / ('lib%d.bam' % (k + 1))))
        bam_writer.write_bam(bams[-1], batch, block_bytes=50000 + 7000 * k, align_records=bool(k % 2))
    return fasta, bams


@pytest.mark.parametrize('name', FU.SCENARIOS)
def test_cli_three_libraries_equal_the_reference(name, files, fixed_uid, tmp_path):
    from besst_amd import cli
    doc = FU.load_doc(name)
    argv, per_lib = FU.cli_args(doc['scenario'], files[0], files[1], str(tmp_path))
    if not per_lib:
        assert cli.main(argv) == 0
    else:
        args = cli.build_parser().parse_args(argv)
        for dest, values in per_lib.items():
            setattr(args, dest, values)
        assert cli._run(args, 0) == 0
    FU.assert_files_equal_fixture(str(tmp_path / 'BESST_output'), doc, name)


def test_cli_two_ranks_write_the_same_files(files, tmp_path):
    """scenario A under torchrun, two gloo ranks on one GPU: rank 0 writes the files of the one-process run (the uid in the
    scaffold names is the child's clock and is set to the fixture's before comparing)"""
    import socket
    doc = FU.load_doc('flow_a')
    argv, per_lib = FU.cli_args(doc['scenario'], files[0], files[1], str(tmp_path))
    assert not per_lib
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, BESST_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), '-m', 'besst_amd.cli'] + argv
    done = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert done.returncode == 0, done.stdout.decode()[-3000:]
    FU.assert_files_equal_fixture(str(tmp_path / 'BESST_output'), doc, 'flow_a, two ranks', uid=True)
