"""SequenceStore.from_fasta(gzip_on_gpu=True) on gzip files of SEVERAL members: the device's parallel inflate
(csrc/gzip_stream.hip, besst_dev_gzip_members_*) against the parser on the plain bytes and against
the model of the scheme (tests/gzip_members_model.py) - the same numbers of chunks, candidates, live segments, members and
member candidates, exactly.  The files are the designed ones of tests/gzip_members_design.py
(tests/test_gzip_members_model.py asserts on the CPU that each holds its border).  A file the device gives up on must reach
the host path - its text, or its FastaError word for word - with the device's reason in ``inflate_stats``; on none of the
good files may the device give up."""
import gzip
import os
import types

import pytest

from besst_amd import GenerateOutput as GO
from tests import flow_util as FLOW
from tests import gzip_members_design as G
from tests import gzip_members_model as MM
from tests import gzip_stream_design as D
from tests import gzip_stream_model as M
from tests.test_gpu_gzip_stream import file_parse, plain_parse, read, run_cli, tree, write

pytestmark = pytest.mark.gpu

PAD = GO.EMIT_PAD
NAMES = sorted(G.files())
KEYS = ('chunks', 'candidates', 'live', 'text_bytes', 'status', 'members', 'member_candidates')


def counts(stats):
    return {k: stats[k] for k in KEYS}


def modelled_counts(model, text):
    return dict(chunks=model['chunks'], candidates=model['candidates'], live=model['live'], text_bytes=len(text), status='ok',
                members=model['members'], member_candidates=model['member_candidates'])


def device_inflate(path, chunk):
    """_upload_gzip_device -> (the text's bytes or None, stats)"""
    import torch
    stats = {}
    got = GO._upload_gzip_device(torch, torch.device('cuda', 0), path, chunk, stats)
    if got is None:
        return None, stats
    out, n = got
    assert out.shape[0] == n + PAD and out[n:].count_nonzero().item() == 0
    return out[:n].cpu().numpy().tobytes(), stats


# ---- 1., 2. every designed file at every chunk size ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in NAMES if G.files()[n][2]])
def test_designed_files(name, tmp_path):
    data, text, _fasta = G.files()[name]
    path = write(tmp_path / 'x.fa.gz', data)
    want = plain_parse(text)
    assert not isinstance(want, tuple)
    for chunk in G.CHUNKS:
        got, inflate, stats = file_parse(path, gzip_on_gpu=True, gzip_chunk_bytes=chunk)
        assert (inflate, stats['status']) == ('device_gzip', 'ok'), (chunk, stats)
        assert got == want, chunk
        assert counts(stats) == modelled_counts(G.modelled(name, chunk), text), chunk
        assert 'bad_member' not in stats and 'bad_member_offset' not in stats


@pytest.mark.parametrize('name', NAMES)
def test_designed_files_text(name, tmp_path):
    """the inflated text itself, byte for byte, whether or not it is a FASTA file"""
    data, text, _fasta = G.files()[name]
    path = write(tmp_path / 'x.gz', data)
    for chunk in G.CHUNKS:
        got, stats = device_inflate(path, chunk)
        assert counts(stats) == modelled_counts(G.modelled(name, chunk), text), chunk
        assert got == text, chunk


# ---- 3. reach, damage, capacity ------------------------------------------------------------------------------------------------------
def test_a_match_reaches_its_member_s_first_byte_and_no_further(tmp_path):
    data, text, _ = G.files()['reach_ok']
    bad, at = G.reach_bad()
    for chunk in G.CHUNKS:
        got, stats = device_inflate(write(tmp_path / 'ok.gz', data), chunk)
        assert stats['status'] == 'ok' and got == text and got[-259:] == b'A' * 259, chunk
        got, stats = device_inflate(write(tmp_path / 'bad.gz', bad), chunk)
        assert got is None and stats['status'] == 'bad_distance', (chunk, stats)
        assert (stats['members'], stats['text_bytes']) == (2, len(text) - 1), chunk       # (the plan found nothing wrong)
    path = write(tmp_path / 'bad.fa.gz', bad)
    with pytest.raises(GO.FastaError, match='invalid distance too far back') as host:
        GO.SequenceStore.from_fasta(path)
    with pytest.raises(GO.FastaError) as dev:
        GO.SequenceStore.from_fasta(path, gzip_on_gpu=True, gzip_chunk_bytes=1024)
    assert (str(dev.value), dev.value.offset) == (str(host.value), host.value.offset) and dev.value.offset == at == 33781
    assert dev.value.inflate_stats['status'] == 'bad_distance'


@pytest.mark.parametrize('how', G.DAMAGE)
def test_damage_reaches_the_host_s_error(how, tmp_path):
    data, status, at = G.damaged()[how]
    path = write(tmp_path / 'bad.fa.gz', data)
    with pytest.raises(GO.FastaError) as host:
        GO.SequenceStore.from_fasta(path)
    assert host.value.offset == at
    for chunk in G.CHUNKS:
        with pytest.raises(GO.FastaError) as dev:
            GO.SequenceStore.from_fasta(path, gzip_on_gpu=True, gzip_chunk_bytes=chunk)
        assert (str(dev.value), dev.value.offset) == (str(host.value), host.value.offset), chunk
        stats = dev.value.inflate_stats
        assert stats['status'] in GO.GZIP_STATUS[1:] and (status is None or stats['status'] == status), (chunk, stats)
        model = MM.FileModel(data).inflate(chunk)
        assert (stats['bad_member'], stats['bad_member_offset']) == (model['bad_member'], model['bad_member_offset']), chunk
        assert stats['bad_member_offset'] == at, chunk


def test_capacity_of_the_member_list(tmp_path, monkeypatch):
    data, text, _ = G.files()['plain_then_bgzf_256']
    path = write(tmp_path / 'many.fa.gz', data)
    want = plain_parse(text)
    n = G.modelled('plain_then_bgzf_256', 1024)['member_candidates']
    monkeypatch.setattr(GO, 'GZIP_MEMBER_CAPACITY', n - 2)
    got, inflate, stats = file_parse(path, gzip_on_gpu=True, gzip_chunk_bytes=1024)
    assert (got, inflate) == (want, 'host') and (stats['status'], stats['member_candidates']) == ('too_many_members', n)
    monkeypatch.setattr(GO, 'GZIP_MEMBER_CAPACITY', n)
    for chunk in G.CHUNKS:
        got, inflate, stats = file_parse(path, gzip_on_gpu=True, gzip_chunk_bytes=chunk)
        assert (got, inflate, stats['status']) == (want, 'device_gzip', 'ok'), chunk
        assert counts(stats) == modelled_counts(G.modelled('plain_then_bgzf_256', chunk), text), chunk


# ---- 4. the one-member streams through the member-aware entry points ---------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(D.streams()))
def test_one_member_streams_keep_their_numbers(name, tmp_path):
    raw, text = D.streams()[name]
    path = write(tmp_path / 'x.gz', M.gzip_member(raw, text))
    for chunk in D.CHUNKS:
        model = D.modelled(name, chunk)
        got, stats = device_inflate(path, chunk)
        assert got == text, chunk
        assert counts(stats) == dict(chunks=model['chunks'], candidates=model['candidates'], live=model['live'],
                                     text_bytes=len(text), status='ok', members=1,
                                     member_candidates=len(MM.member_candidates(M.gzip_member(raw, text)))), chunk


# ---- 5. the command line ---------------------------------------------------------------------------------------------------------------
def test_cli_reads_a_gzip_fasta_of_three_members_on_the_gpu(tmp_path, monkeypatch):
    """scenario A from contigs.fa.gz written as three members, with --fasta_on_gpu --gzip_on_gpu: the files of the run from
    contigs.fa"""
    from tests import bam_writer
    asm, libs = FLOW.load_inputs()
    fasta = FLOW.write_fasta(str(tmp_path / 'contigs.fa'), FLOW.contig_sequences(asm))
    plain = read(fasta)
    a, b = len(plain) // 3, 2 * len(plain) // 3 + 5
    packed = write(tmp_path / 'contigs.fa.gz', gzip.compress(plain[:a], 6) + gzip.compress(plain[a:b], 1) + gzip.compress(plain[b:], 9))
    bams = []
    for k, batch in enumerate(libs):
        bams.append(str(tmp_path / ('lib%d.bam' % (k + 1))))
        bam_writer.write_bam(bams[-1], batch, block_bytes=50000 + 7000 * k, align_records=bool(k % 2))
    monkeypatch.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FLOW.UNIQUE_ID)))
    want = tree(run_cli(fasta, bams, str(tmp_path / 'plain'), ['--fasta_on_gpu']))
    seen, real = [], GO._upload_gzip_device

    def spy(*args):
        got = real(*args)
        seen.append((got is not None, args[4]['status'], args[4]['members']))
        return got
    monkeypatch.setattr(GO, '_upload_gzip_device', spy)
    out = run_cli(packed, bams, str(tmp_path / 'gz'), ['--fasta_on_gpu', '--gzip_on_gpu'])
    assert seen == [(True, 'ok', 3)]
    assert tree(out) == want and any(k.endswith('Scaffolds-pass3.fa') for k in want)
    assert os.path.getsize(packed) < len(plain)
