"""The contig FASTA on the device (csrc/fasta.hip) against tests/fasta_util.py's plain-Python model and the fixture taken
from the reference's ReadInContigseqs: through the C ABI (GenerateOutput.parse_fasta_text on a device buffer), through
SequenceStore.from_fasta on a file, and through the command line's --fasta_on_gpu / -filter_contigs.

Tile sizes: 1024 bytes (the smallest accepted, so that a few KiB hold many tile borders) and the default."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from besst_amd import GenerateOutput as GO
from tests import fasta_util as FU
from tests import flow_util as FLOW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 1024
TILES = (SMALL, None)
PAD = GO.EMIT_PAD


def device_text(data):
    import torch
    t = torch.zeros(len(data) + PAD, dtype=torch.uint8, device='cuda')
    if data:
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return t


def device_parse(data, tile):
    """-> dict(names, offsets, lengths, pool) as Python values, or ('error', offset)"""
    try:
        out = GO.parse_fasta_text(device_text(data), len(data), tile)
    except GO.FastaError as exc:
        return ('error', exc.offset)
    n = out['pool_bytes']
    blob, at = out['names'].cpu().numpy().tobytes().decode('ascii'), out['name_off'].cpu().tolist()
    assert out['pool'][:PAD].count_nonzero().item() == 0 and out['pool'][PAD + n:].count_nonzero().item() == 0
    return dict(names=[blob[a:b] for a, b in zip(at[:-1], at[1:])], offsets=out['ctg_off'].cpu().tolist(),
                lengths=out['ctg_len'].cpu().tolist(), pool=out['pool'][PAD:PAD + n].cpu().numpy().tobytes())


def model_parse(data):
    try:
        rows = FU.parse_rows(data)
    except FU.FastaError as exc:
        return ('error', exc.offset)
    pool, offsets, lengths = FU.pool_of(rows)
    return dict(names=[name for name, _ in rows], offsets=offsets, lengths=lengths, pool=pool)


def assert_same(data, tile, what):
    got, want = device_parse(data, tile), model_parse(data)
    if isinstance(want, tuple) or isinstance(got, tuple):
        assert got == want, what
        return
    for key in ('names', 'lengths', 'offsets'):
        assert got[key] == want[key], (what, key)
    assert got['pool'] == want['pool'], (what, 'pool')


# ---- 1. the fixture ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def golden():
    return FU.load_golden()


@pytest.mark.parametrize('tile', TILES)
def test_fixture_cases(golden, tile, tmp_path):
    for case in golden['cases']:
        want = case['expect']
        path = str(tmp_path / 'case.fa')
        with open(path, 'wb') as fh:
            fh.write(case['data'])
        if want.get('error') in ('IndexError', 'UnicodeDecodeError'):
            with pytest.raises(ValueError):
                GO.SequenceStore.from_fasta(path, tile_bytes=tile)
            assert isinstance(device_parse(case['data'], tile), tuple)
            continue
        assert_same(case['data'], tile, case['name'])
        with GO.SequenceStore.from_fasta(path, tile_bytes=tile) as store:
            full, _ = FU.read_contigs(case['data'])
            if 'contigs' in want and not case['filter']:
                assert [list(kv) for kv in full.items()] == want['contigs']
            cd = store.contig_dict()
            assert [(k, str(v)) for k, v in cd.items()] == list(full.items()), case['name']   # order, duplicates, bytes
            assert [len(v) for v in cd.values()] == [len(v) for v in full.values()]
            assert all(store.names[store.index[k]] == k for k in cd)
            import io
            info = io.StringIO()
            kept = store.contig_dict(case['filter'], info)
            model, text = FU.read_contigs(case['data'], case['filter'])
            assert ([(k, str(v)) for k, v in kept.items()], info.getvalue()) == (list(model.items()), text), case['name']
            if 'contigs' in want:
                assert ([list(kv) for kv in model.items()], text) == (want['contigs'], want['info']), case['name']


# ---- 2. every interesting byte on every position relative to a tile border -------------------------------------------------
def sweep_body():
    body = (b'ACGTACGT\r\nTTGA\rGG>CC\n>c1 a comment that goes on\nACGTNN  \t\n\nAC GT\n' + b'ACGTTGCA' * 7 + b'\n') * 2
    body += b'>c2\tx\r\n' + b'GATTACA' * 30 + b' \r\n\r\n  TT  \n>c3\n'
    while len(body) < 3 * SMALL:
        body += b'ACGTACGTAC' * 6 + b'\n'
    return body + b'GG \t'


def test_boundary_sweep():
    body = sweep_body()
    assert 3 * SMALL <= len(body) < 3 * SMALL + 80
    for k in range(0, SMALL + 17):
        assert_same(b'>c0 x\n' + b'A' * k + b'\n' + body, SMALL, 'k = %d' % k)


# ---- 3. long lines -----------------------------------------------------------------------------------------------------
LONG = {
    'one line, no newline at the end': b'>c\n' + b'ACGTT' * SMALL + b'ACG',
    'trailing blanks over three tiles': b'>c\nACGT' + b' \t' * (2 * SMALL) + b'\nTT\n>d\nGG\n',
    'trailing blanks over three tiles, end of file': b'>c\nACGT' + b' ' * (4 * SMALL),
    'leading blanks over three tiles': b'>c\n' + b'\x1c ' * (2 * SMALL) + b'ACGT\nTT\n',
    'blank line over three tiles': b'>c\nAC\n' + b' ' * (4 * SMALL) + b'\nGT\n',
    'interior blanks over three tiles': b'>c\nAC' + b' ' * (4 * SMALL) + b'GT\n',
    'header comment over three tiles': b'>c1 ' + b'comment ' * (SMALL // 2) + b'\nACGT\n>c2\nTT\n',
    'name across a tile border': b'>a\n' + b'A' * (SMALL - 10) + b'\n>name_across_the_border rest\nACGT\n',
    'name longer than a tile': b'>' + b'n' * (SMALL + 100) + b' x\nACGT\n',
    'blanks before a name across a border': b'>a\n' + b'A' * (SMALL - 8) + b'\n>   \t  name\nAC\n',
}
assert len(LONG['one line, no newline at the end']) == 5 * SMALL + 3 + 3


@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('what', sorted(LONG))
def test_long_lines(what, tile):
    assert_same(LONG[what], tile, what)


# ---- 4. random texts ---------------------------------------------------------------------------------------------------
def test_random_differential():
    rejected = 0
    for seed in range(300):
        data = FU.random_text(seed)
        want = model_parse(data)
        rejected += isinstance(want, tuple)
        for tile in TILES:
            assert_same(data, tile, 'seed %d, tile %s' % (seed, tile))
    assert 20 <= rejected <= 200                                 # both kinds of text occur


# ---- 5. the 16-byte stores: every residue of a contig's pool offset -------------------------------------------------------
@pytest.mark.parametrize('tile', TILES)
def test_output_alignment(tile):
    rng = np.random.default_rng(5)
    data = b''
    for rounds in range(3):
        for n in range(34):
            seq = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
            data += b'>k%d_%d\n' % (rounds, n) + seq + b'\n'
    want = model_parse(data)
    assert {o % 16 for o in want['offsets']} == set(range(16))
    assert_same(data, tile, 'alignment')


# ---- 6. errors are a status ------------------------------------------------------------------------------------------------
def test_errors_and_recovery():
    good = b'>a\n' + b'ACGT' * 700 + b'\n>b\nTT\n'
    bad = bytearray(good)
    bad[2 * SMALL + 5], bad[SMALL - 3] = 0xC3, 0x80
    for tile in TILES:
        assert device_parse(bytes(bad), tile) == ('error', SMALL - 3)
        nameless = b'>a\nACGT\n' + b'A' * SMALL + b'\n> \t\nTT\n>\n'
        assert device_parse(nameless, tile) == ('error', 8 + SMALL + 1)
        with pytest.raises(ValueError, match='byte %d ' % (8 + SMALL + 1)):
            GO.parse_fasta_text(device_text(nameless), len(nameless), tile)
        assert_same(good, tile, 'after the errors')


# ---- 7. offsets past 2^32 ----------------------------------------------------------------------------------------------
def test_past_four_gigabytes():
    import torch
    tile = 16384
    n = (1 << 32) + 2 * tile + 123
    text = torch.full((n + PAD,), 65, dtype=torch.uint8, device='cuda')
    text[n:] = 0

    def put(at, data):
        text[at:at + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()

    breaks = [1400000007, 2800000011, (1 << 32) - 2, n - 50]      # the '\n' in front of every later header
    put(0, b'>a\n')
    for at, name in zip(breaks, b'bcde'):
        put(at, b'\n>' + bytes([name]) + b'\n')
    starts = [3] + [at + 4 for at in breaks]                     # first base of every contig, in the file
    ends = breaks + [n]
    lengths = [e - s for s, e in zip(starts, ends)]
    offsets = [0] + np.cumsum(lengths)[:-1].tolist()
    assert max(lengths) < 1 << 31 and breaks[2] < 1 << 32 < breaks[2] + 4
    out = GO.parse_fasta_text(text, n, tile)
    assert out['pool_bytes'] == n - 3 - 4 * len(breaks) == sum(lengths)
    assert out['ctg_len'].cpu().tolist() == lengths and out['ctg_off'].cpu().tolist() == offsets
    assert out['names'].cpu().numpy().tobytes() == b'abcde' and out['name_off'].cpu().tolist() == [0, 1, 2, 3, 4, 5]
    pool = out['pool'][PAD:PAD + out['pool_bytes']]
    assert not bool((pool != 65).any())
    del out, pool
    for at in breaks[:2]:
        put(at, b'AAAA')
    with pytest.raises(ValueError, match='2\\^31 bases or more'):
        GO.parse_fasta_text(text, n, tile)


# ---- 8. the store, and the command line ------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """contigs.fa and lib1..3.bam of the flow fixture's inputs, written once"""
    from tests import bam_writer
    asm, libs = FLOW.load_inputs()
    d = tmp_path_factory.mktemp('fasta_inputs')
    fasta = FLOW.write_fasta(str(d / 'contigs.fa'), FLOW.contig_sequences(asm))
    bams = []
    for k, batch in enumerate(libs):
        bams.append(str(d / ('lib%d.bam' % (k + 1))))
        bam_writer.write_bam(bams[-1], batch, block_bytes=50000 + 7000 * k, align_records=bool(k % 2))
    return fasta, bams


@pytest.fixture
def fixed_uid(monkeypatch):
    monkeypatch.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FLOW.UNIQUE_ID)))


def test_store_from_fasta_equals_the_constructor(files):
    import torch
    asm, _ = FLOW.load_inputs()
    seqs = FLOW.contig_sequences(asm)
    for tile in TILES:
        with GO.SequenceStore(list(seqs), list(seqs.values())) as want, \
                GO.SequenceStore.from_fasta(files[0], tile_bytes=tile) as got:
            assert got.index == want.index and got.names == list(seqs)
            assert got.offsets.tolist() == want.offsets.tolist() and got.offsets.dtype == want.offsets.dtype
            assert got.lengths.tolist() == want.lengths.tolist() and got.lengths.dtype == want.lengths.dtype
            assert (got.pool_bytes, len(got)) == (want.pool_bytes, len(want))
            assert torch.equal(got._pool, want._pool) and torch.equal(got._off, want._off) and torch.equal(got._len, want._len)
            assert got.pool_ptr == got._pool.data_ptr() + PAD
            row = len(got) // 2
            assert got.fetch(row).decode() == seqs[got.names[row]]


def run_cli(name, files, out, extra):
    from besst_amd import cli
    doc = FLOW.load_doc(name)
    argv, per_lib = FLOW.cli_args(doc['scenario'], files[0], files[1], out)
    args = cli.build_parser().parse_args(argv + extra)
    for dest, values in per_lib.items():
        setattr(args, dest, values)
    assert cli._run(args, 0) == 0
    return doc


def read(path):
    with open(path, 'rb') as fh:
        return fh.read()


@pytest.mark.parametrize('name', FLOW.SCENARIOS)
def test_cli_reads_the_fasta_on_the_gpu(name, files, fixed_uid, tmp_path, monkeypatch):
    from besst_amd import cli
    monkeypatch.setattr(cli, 'read_fasta', None)                 # not called on this path
    doc = run_cli(name, files, str(tmp_path / 'gpu'), ['--fasta_on_gpu'])
    FLOW.assert_files_equal_fixture(str(tmp_path / 'gpu' / 'BESST_output'), doc, name)
    monkeypatch.undo()
    if doc['scenario']['cov_cutoff'] is None:
        return
    # the scenario with -z: contigs are dropped as repeats and for low coverage, and their bases are written from handles
    monkeypatch.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FLOW.UNIQUE_ID)))
    run_cli(name, files, str(tmp_path / 'host'), [])
    sizes = []
    for fname in ('repeats.fa', 'low_coverage_contigs.fa'):
        a, b = (read(str(tmp_path / d / 'BESST_output' / fname)) for d in ('gpu', 'host'))
        assert a == b, fname
        sizes.append(len(a))
    assert max(sizes) > 0


def test_cli_two_ranks_read_the_fasta_on_the_gpu(files, tmp_path):
    import socket
    doc = FLOW.load_doc('flow_a')
    argv, per_lib = FLOW.cli_args(doc['scenario'], files[0], files[1], str(tmp_path))
    assert not per_lib
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, BESST_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), '-m', 'besst_amd.cli'] + argv + ['--fasta_on_gpu']
    done = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert done.returncode == 0, done.stdout.decode()[-3000:]
    FLOW.assert_files_equal_fixture(str(tmp_path / 'BESST_output'), doc, 'flow_a, two ranks', uid=True)


# ---- 9. -filter_contigs ------------------------------------------------------------------------------------------------
def test_filter_contigs_on_both_paths(files, fixed_uid, tmp_path):
    from besst_amd import cli
    asm, _ = FLOW.load_inputs()
    lengths = sorted(int(x) for x in asm['lengths'])
    threshold = lengths[len(lengths) // 8] + 1                   # an eighth of the contigs of the BAM header go
    dropped = [n for n, l in zip(asm['names'], asm['lengths']) if l < threshold]
    assert 0 < len(dropped) < len(lengths) // 4
    model, info = FU.read_contigs(read(files[0]), threshold)
    assert len(model) == len(lengths) - len(dropped) and not set(dropped) & set(model)
    host = GO.filter_contigs(cli.read_fasta(files[0]), threshold)
    with GO.SequenceStore.from_fasta(files[0]) as store:
        device = store.contig_dict(threshold)
        assert list(device) == list(host) == list(model)
        assert [len(v) for v in device.values()] == [len(v) for v in model.values()]
    outs = {}
    for key, extra in (('host', []), ('gpu', ['--fasta_on_gpu'])):
        out = str(tmp_path / key)
        run_cli('flow_a', files, out, extra + ['-filter_contigs', str(threshold)])
        stats = read(os.path.join(out, 'BESST_output', 'Statistics.txt')).decode()
        assert info in stats, key                                # both lines, in the reference's words
        outs[key] = {}
        for dirpath, _dirs, fnames in os.walk(os.path.join(out, 'BESST_output')):
            for fname in fnames:
                if fname != 'Statistics.txt':
                    outs[key][os.path.relpath(os.path.join(dirpath, fname), out)] = read(os.path.join(dirpath, fname))
        assert any(k.endswith('Scaffolds-pass3.fa') for k in outs[key]) and any(k.endswith('.agp') for k in outs[key])
        import re
        for path, content in outs[key].items():
            if path.endswith(('.agp', '.gff', '.tsv', '.fa')):
                words = set(re.split(r'[\s;=>]+', content.decode()))
                assert not words & set(dropped), (key, path)
    assert outs['host'] == outs['gpu']
