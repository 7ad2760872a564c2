"""No GPU: the SAM entry points are bound and answer argument errors, bamio.open_bam tells BAM from SAM by content
(through bamio.reader_class, which touches no device), the header parser's rules, and the command line's refusal of a SAM
file under a process group - before any group is formed."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from besst_amd import _lib, bamio
from tests import bgzf_writer, sam_design

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAM = os.path.join(ROOT, 'tests', 'golden', 'sam', 'handmade.sam')
BAM = os.path.join(ROOT, 'tests', 'golden', 'bam', 'handmade_a.bam')


def test_entry_points_are_bound():
    lib = _lib.load()
    for name in ('besst_ctx_set_sam_references', 'besst_dev_sam_workspace_bytes', 'besst_ctx_push_sam_text'):
        assert name in _lib._SIGNATURES and getattr(lib, name) is not None
    assert lib.besst_abi_version() == 3


def test_argument_errors_need_no_gpu():
    lib = _lib.load()
    info = np.zeros(4, dtype=np.int64)
    text = np.zeros(4096 + 64, dtype=np.uint8)
    at = text.ctypes.data + (-text.ctypes.data) % 16
    assert lib.besst_ctx_push_sam_text(None, None, at, 1024, 0, 0, 0, None, None, None, _lib.ptr(info)) == 1
    assert 'null context' in _lib.last_error()
    assert lib.besst_ctx_set_sam_references(None, None, None, 0) == 1
    assert 'null context' in _lib.last_error()
    # the size, tile and alignment checks come before the context is looked at: a block of zero bytes stands in for one
    stand_in = np.zeros(8192, dtype=np.uint8)
    for tile in (1000, 512, 65536 + 1024, -1024):
        assert lib.besst_ctx_push_sam_text(_lib.ptr(stand_in), None, at, 1024, 0, tile, 0, None, None, None, _lib.ptr(info)) == 1
        assert 'tile_bytes' in _lib.last_error()
        assert lib.besst_dev_sam_workspace_bytes(1 << 20, tile) == 0
    assert lib.besst_ctx_push_sam_text(_lib.ptr(stand_in), None, at + 4, 1024, 0, 1024, 0, None, None, None, _lib.ptr(info)) == 1
    assert '16-byte aligned' in _lib.last_error()
    assert lib.besst_ctx_push_sam_text(_lib.ptr(stand_in), None, at, 1 << 32, 0, 1024, 0, None, None, None, _lib.ptr(info)) == 1
    small, large = lib.besst_dev_sam_workspace_bytes(1 << 20, 0), lib.besst_dev_sam_workspace_bytes(1 << 20, 1024)
    assert 0 < small < large and lib.besst_dev_sam_workspace_bytes(1 << 20, 16384) == small


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp('sniff')
    with open(SAM, 'rb') as fh:
        sam = fh.read()
    with open(BAM, 'rb') as fh:
        bam = fh.read()
    out = {}

    def put(name, data):
        out[name] = str(d / name)
        with open(out[name], 'wb') as fh:
            fh.write(data)
    put('plain.bam', sam)                                        # (the names lie on purpose: the content decides)
    put('bgzf_sam.bam', bgzf_writer.bgzf(sam, payload=700))
    put('eof_block_first.sam.gz', bgzf_writer.bgzf(sam, payload=700, empty_at=(0,)))
    put('gzip_sam.txt', gzip.compress(sam))
    put('no_header.sam', sam[sam.index(b'r01_plain'):])
    put('real_bam.sam', bam)
    put('damaged_bam.sam', bgzf_writer.damaged(bam, 0, 'payload')[0])
    put('damaged_bgzf_sam.sam', bgzf_writer.damaged(bgzf_writer.bgzf(sam, payload=700), 0, 'payload')[0])
    put('cut_bam.bam', bgzf_writer.damaged(bam, 0, 'cut')[0])
    put('empty.sam', b'')
    return out


@pytest.mark.parametrize('name,want', [('plain.bam', 'ResidentSam'), ('bgzf_sam.bam', 'ResidentSam'),
                                       ('eof_block_first.sam.gz', 'ResidentSam'), ('gzip_sam.txt', 'ResidentSam'),
                                       ('no_header.sam', 'ResidentSam'), ('real_bam.sam', 'ResidentBam'),
                                       ('damaged_bam.sam', 'ResidentBam'), ('damaged_bgzf_sam.sam', 'ResidentBam'),
                                       ('cut_bam.bam', 'ResidentBam'), ('empty.sam', 'ResidentSam')])
def test_format_is_told_by_content(files, name, want):
    assert bamio.reader_class(files[name]).__name__ == want


def test_existing_bam_fixtures_stay_bam():
    for name in ('handmade_a.bam', 'handmade_b.bam'):
        assert bamio.reader_class(os.path.join(ROOT, 'tests', 'golden', 'bam', name)) is bamio.ResidentBam


def test_header_parsing():
    names, lengths = bamio.parse_sam_header([b'@HD\tVN:1.4\n', b'@SQ\tSN:a\tLN:5\n', b'@CO\tSN:x\tLN:1\n',
                                             b'@SQ\tLN:70\tAS:asm\tSN:b c\r\n', b'@SQ\tM5:0\tSN:c\tUR:file\tLN:2147483647'])
    assert (names, lengths) == (['a', 'b c', 'c'], [5, 70, 2147483647])
    assert bamio.parse_sam_header([b'@HD\tVN:1.4\n', b'@PG\tID:x\n']) == ([], [])
    assert bamio.parse_sam_header([]) == ([], [])
    assert bamio.parse_sam_header([b'@SQ\tSN:a\tLN:0\n']) == (['a'], [0])      # (a BAM header may say 0)
    with pytest.raises(bamio.SamError) as err:
        bamio.parse_sam_header([b'@SQ\tSN:a\tLN:5\n', b'@SQ\tSN:b\tLN:6\n', b'@SQ\tLN:7\tSN:a\n'])
    assert (err.value.offset, err.value.line) == (28, 3) and 'repeats' in str(err.value)
    for bad in (b'@SQ\tSN:a\n', b'@SQ\tLN:5\n', b'@SQ\tSN:\tLN:5\n', b'@SQ\tSN:a\tLN:x\n', b'@SQ\tSN:a\tLN:-1\n',
                b'@SQ\tSN:a\tLN:2147483648\n'):
        with pytest.raises(bamio.SamError) as err:
            bamio.parse_sam_header([b'@HD\tVN:1\n', bad])
        assert (err.value.offset, err.value.line) == (9, 2)
    assert issubclass(bamio.SamError, ValueError)
    with open(SAM, 'rb') as fh:
        lines, size = bamio._read_plain_header(fh)
        assert fh.read(9) == b'r01_plain'
    assert len(lines) == 4 and size == sum(len(l) for l in lines)
    assert bamio.parse_sam_header(lines) == (['ctgA', 'ctgB', 'a_rather_long_reference_name_to_cross_a_block_boundary'],
                                             [5000, 12345, 70000])
    assert bamio.parse_sam_header(sam_design.header_bytes().splitlines(True)) == (sam_design.REFS, sam_design.LENGTHS)


def test_reason_table_matches_the_header_file():
    text = open(os.path.join(ROOT, 'include', 'besst_amd.h')).read()
    import re
    codes = {name: int(v) for name, v in re.findall(r'#define BESST_SAM_(\w+) (\d+)', text) if name != 'INFO_WORDS'}
    assert sorted(codes.values()) == sorted(bamio.SAM_REASONS) == list(range(1, 12))
    assert 'eleven' in bamio.SAM_REASONS[codes['FEW_FIELDS']] and 'CIGAR' in bamio.SAM_REASONS[codes['BAD_CIGAR']]


def test_cli_refuses_sam_under_a_process_group(files, tmp_path):
    """WORLD_SIZE=2 in a child process: the exit comes before join_process_group - no master address is set, so forming a
    group could only fail otherwise - with the message that names BAM as the sharded input."""
    fasta = str(tmp_path / 'contigs.fa')
    with open(fasta, 'w') as fh:
        fh.write('>ctgA\nACGT\n')
    env = dict(os.environ, WORLD_SIZE='2', RANK='1', LOCAL_RANK='1', PYTHONPATH=ROOT)
    for key in ('MASTER_ADDR', 'MASTER_PORT'):
        env.pop(key, None)
    for name in ('plain.bam', 'gzip_sam.txt'):
        ran = subprocess.run([sys.executable, '-m', 'besst_amd.cli', '-c', fasta, '-f', BAM, files[name], '-orientation', 'fr', 'fr',
                              '-o', str(tmp_path / 'out')], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
        assert ran.returncode == 1, ran.stderr[-2000:]
        assert files[name] in ran.stderr and 'BAM' in ran.stderr and 'process group' in ran.stderr
        assert not os.path.exists(str(tmp_path / 'out'))


def test_gzip_on_gpu_is_tied_to_the_fasta_unless_a_sam_is_compressed(files, tmp_path, monkeypatch):
    from besst_amd import cli
    monkeypatch.setattr(cli, 'join_process_group', lambda: (_ for _ in ()).throw(RuntimeError('reached the run')))
    common = ['-c', SAM, '-orientation', 'fr', '-o', str(tmp_path), '--gzip_on_gpu']
    for name in ('plain.bam', 'real_bam.sam'):
        with pytest.raises(SystemExit) as err:
            cli.main(common + ['-f', files[name]])
        assert '--fasta_on_gpu' in str(err.value)
    for name in ('gzip_sam.txt', 'bgzf_sam.bam'):
        with pytest.raises(RuntimeError, match='reached the run'):
            cli.main(common + ['-f', files[name]])
