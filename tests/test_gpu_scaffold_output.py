"""The scaffold output stage on the device (csrc/emit.hip behind besst_amd.GenerateOutput): every case of the fixture
captured from the reference, byte for byte; the overlap kernel on every junction; chunked emission; every source and
destination alignment; an assembly past 1 GB; one store under two placements; the CLI end to end."""
import collections
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from besst_amd import GenerateOutput as GO
from besst_amd import _lib
from tests import output_util as OU

pytestmark = pytest.mark.gpu

DOC = OU.load_golden()
CASES = {c['name']: c for c in DOC['cases']}
UID = DOC['unique_id']


def _param(case, out_dir=None):
    return OU.Param(case['K'], case['sigma'], None if out_dir is None else str(out_dir), io.StringIO())


@pytest.mark.parametrize('name', sorted(CASES))
def test_print_output_equals_the_reference(name, tmp_path):
    case, want = CASES[name], CASES[name]['expect']
    param, info = _param(case, tmp_path), io.StringIO()
    F = OU.case_F(case)
    if want['key_error'] is not None:
        with pytest.raises(KeyError) as exc:
            GO.PrintOutput(F, info, str(tmp_path), param, 1, unique_id=UID)
        assert exc.value.args == (want['key_error'],)
        assert os.listdir(str(tmp_path / 'pass1')) == []          # nothing is written
    else:
        assert GO.PrintOutput(F, info, str(tmp_path), param, 1, unique_id=UID) == ()
        for key, fname in (('fasta', 'Scaffolds-pass1.fa'), ('agp', 'info-pass1.agp'), ('gff', 'info-pass1.gff')):
            with open(str(tmp_path / 'pass1' / fname), newline='') as fh:
                assert fh.read() == want[key], key
        assert sorted(os.listdir(str(tmp_path / 'pass1'))) == ['Scaffolds-pass1.fa', 'info-pass1.agp', 'info-pass1.gff']
        assert GO.scaffold_bytes(F, _param(case), unique_id=UID) == want['fasta'].encode()
    assert info.getvalue() == want['information']
    assert param.information_file.getvalue().splitlines() == want['merging']


def test_unique_id_defaults_to_the_clock():
    import time
    case = CASES['short_K5']
    t0 = int(time.time())
    text = GO.scaffold_bytes(OU.case_F(case), _param(case)).decode()
    t1 = int(time.time())
    uid = int(text.split('\n', 1)[0].rsplit('_', 1)[1])
    assert text.startswith('>scaffold_1_uid_') and t0 <= uid <= t1


def _junctions(F):
    return [(a, b) for scaf in OU.ordered(F) for a, b in zip(scaf[:-1], scaf[1:])]


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_seq_overlaps_on_every_junction(name):
    case = CASES[name]
    F = OU.case_F(case)
    flat = [t for scaf in OU.ordered(F) for t in scaf]
    row_of = {id(t): i for i, t in enumerate(flat)}
    pairs = _junctions(F)
    if not pairs:
        return                                                   # single-contig scaffolds only
    pool, off, length = GO.pack_sequences([t[4] for t in flat])
    left = np.array([row_of[id(a)] for a, _ in pairs], dtype=np.int32)
    right = np.array([row_of[id(b)] for _, b in pairs], dtype=np.int32)
    forward = np.array([int(a[1]) | (int(b[1]) << 1) for a, b in pairs], dtype=np.uint8)
    got = np.full(len(pairs), -7, dtype=np.int32)
    err = (C.c_uint64 * 1)()
    p = _lib.ptr
    _lib.check(_lib.load().besst_host_seq_overlaps(0, p(pool), len(pool), len(flat), p(off), p(length), len(pairs), p(left),
                                                   p(right), p(forward), case['K'], p(got), err), 'besst_host_seq_overlaps')
    compared, first_bad = 0, None
    for j, (a, b) in enumerate(pairs):
        try:
            want = OU.window_overlap(a, b, case['K'])
        except KeyError:
            continue                                             # a reversed contig without a complement: no overlap to speak of
        assert int(got[j]) == want, (j, a[0], b[0])
        compared += 1
    assert compared >= len(pairs) - 2 and 0 <= int(got.min()) and int(got.max()) <= case['K']
    # the error word: the first junction whose reversed right window holds a byte without a complement
    for j, (a, b) in enumerate(pairs):
        window = b[4][::-1][:case['K']]
        bad = [i for i, ch in enumerate(window) if ch not in OU.COMPLEMENT] if not b[1] else []
        if bad:
            first_bad = (j << 32) | bad[0]
            break
    assert err[0] == (first_bad if first_bad is not None else 0xFFFFFFFFFFFFFFFF)


def _big_F(n_contigs, seed):
    asm = OU.seeded_assembly(n_contigs, 200, 3000, seed)
    pool, off, length = asm['pool'], asm['offsets'], asm['lengths']
    row = {n: i for i, n in enumerate(asm['names'])}
    F = [[(n, d, p, l, pool[off[row[n]]:][:l].tobytes().decode()) for n, d, p, l, _ in scaf] for scaf in asm['F']]
    want = OU.numpy_fasta(asm['scaffolds'], pool, off, length, asm['overlaps'], asm['sigma'], UID).tobytes()
    return asm, F, want


def test_chunked_emission_equals_one_shot():
    """ranges of 1 and 7 bytes on a small case, of 4096 bytes and 1 MB on a 3 MB one: tile and alignment edges"""
    small = CASES['short_K200']
    whole = GO.scaffold_bytes(OU.case_F(small), _param(small), unique_id=UID)
    assert whole == small['expect']['fasta'].encode()
    for step in (1, 7):
        assert GO.scaffold_bytes(OU.case_F(small), _param(small), unique_id=UID, chunk_bytes=step) == whole
    asm, F, want = _big_F(2000, 11)
    assert len(want) > 3 << 20 and len(asm['overlaps']) > 10
    param = OU.Param(200, asm['sigma'], None, io.StringIO())
    whole = GO.scaffold_bytes(F, param, unique_id=UID)
    assert whole == want
    assert len(param.information_file.getvalue().splitlines()) > 5        # planted overlaps merged
    for step in (4096, 1 << 20):
        assert GO.scaffold_bytes(F, OU.Param(200, asm['sigma'], None, io.StringIO()), unique_id=UID, chunk_bytes=step) == whole


def test_every_source_and_destination_alignment():
    """contigs at all 16 pool offsets mod 16 x all 16 output offsets mod 16, both directions, lengths 1..70 - one piece
    table through besst_host_emit_scaffolds, whole and from an odd range start"""
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(b'ACGTNacgtnRYKMSWBVHDX', dtype=np.uint8)
    pool_parts, src, ln, mode, pool_len, out_len = [], [], [], [], 0, 0
    literals = np.frombuffer(b'................\n', dtype=np.uint8)

    def add(s, l, m):
        nonlocal out_len
        src.append(s); ln.append(l); mode.append(m)
        out_len += l

    for length in range(1, 71):
        for a in range(16):
            for b in range(16):
                for m in (GO.PIECE_COPY, GO.PIECE_REVCOMP):
                    pad = (a - pool_len) % 16
                    pool_parts.append(alphabet[rng.integers(0, len(alphabet), pad + length)])
                    fill = (b - out_len) % 16
                    if fill:
                        add(0, fill, GO.PIECE_LITERAL if (a + b) % 3 else GO.PIECE_FILL_N)
                    assert (pool_len + pad) % 16 == a and out_len % 16 == b
                    add(pool_len + pad, length, m)
                    pool_len += pad + length
        add(16, 1, GO.PIECE_LITERAL)
    pool = np.concatenate(pool_parts)
    tab = dict(src_off=np.array(src, np.int64), len=np.array(ln, np.int64), mode=np.array(mode, np.uint8),
               literals=literals, total=out_len)
    tab['out_off'] = np.concatenate(([0], np.cumsum(tab['len']))).astype(np.int64)
    want = OU.apply_pieces(tab, pool)
    lib, p = _lib.load(), _lib.ptr
    for begin, end in ((0, out_len), (5, out_len - 3), (4099, 4099 + 70000)):
        out = np.zeros(end - begin, dtype=np.uint8)
        err = (C.c_uint64 * 2)()
        _lib.check(lib.besst_host_emit_scaffolds(0, p(pool), len(pool), p(literals), len(literals), len(src), p(tab['src_off']),
                                                 p(tab['len']), p(tab['mode']), p(tab['out_off']), begin, end, p(out), err),
                   'besst_host_emit_scaffolds')
        assert out.tobytes() == want[begin:end]
        assert err[0] == err[1] == 0xFFFFFFFFFFFFFFFF


def test_bad_byte_is_a_status_not_a_trap():
    """a reversed piece with bytes that have no complement: the call completes, err[0] names the first"""
    pool = np.frombuffer(b'ACGT' * 10 + b'AC-TU' + b'ACGT' * 10, dtype=np.uint8).copy()
    n = len(pool)
    src, ln = np.array([0, 0], np.int64), np.array([n, n], np.int64)
    mode, off = np.array([GO.PIECE_COPY, GO.PIECE_REVCOMP], np.uint8), np.array([0, n, 2 * n], np.int64)
    out, err = np.zeros(2 * n, np.uint8), (C.c_uint64 * 2)()
    p = _lib.ptr
    _lib.check(_lib.load().besst_host_emit_scaffolds(0, p(pool), n, None, 0, 2, p(src), p(ln), p(mode), p(off), 0, 2 * n,
                                                     p(out), err), 'besst_host_emit_scaffolds')
    assert out[:n].tobytes() == pool.tobytes()
    assert err[0] == (1 << 32) | 40 and err[1] == 0xFFFFFFFFFFFFFFFF     # 'U' is 40 bytes from the end
    good = out[n:].tobytes()
    assert good[:40] == b'ACGT' * 10 and good[45:] == b'ACGT' * 10 and good[40] == 0 and good[42] == 0


def test_sequence_store_serves_two_placements(tmp_path):
    asm = OU.seeded_assembly(300, 50, 900, 3)
    pool, off, length = asm['pool'], asm['offsets'], asm['lengths']
    with OU.store_of(asm) as store:
        assert len(store) == 300 and store.pool_bytes == len(pool)
        for pass_nr, take in ((1, slice(None)), (2, slice(10, 200))):
            # second pass: other scaffolds (a subset, every direction flipped, shifted positions)
            scaffolds = asm['scaffolds'][take]
            if pass_nr == 2:
                scaffolds = [[(r, not d, p + 7, l) for r, d, p, l in s] for s in scaffolds]
            F = [[(asm['names'][r], d, p, l, '') for r, d, p, l in s] for s in reversed(scaffolds)]
            flat = {(k, i): OU.window_overlap((0, a[1], 0, 0, pool[off[a[0]]:][:length[a[0]]].tobytes().decode()),
                                              (0, b[1], 0, 0, pool[off[b[0]]:][:length[b[0]]].tobytes().decode()), 200)
                    for k, s in enumerate(scaffolds) for i, (a, b) in enumerate(zip(s[:-1], s[1:]))}
            want = OU.numpy_fasta(scaffolds, pool, off, length, flat, asm['sigma'], UID).tobytes()
            param = OU.Param(200, asm['sigma'], str(tmp_path), io.StringIO())
            GO.PrintOutput(F, io.StringIO(), str(tmp_path), param, pass_nr, store=store, unique_id=UID)
            with open(str(tmp_path / ('pass%d' % pass_nr) / ('Scaffolds-pass%d.fa' % pass_nr)), 'rb') as fh:
                assert fh.read() == want


def test_assembly_past_one_gigabyte(tmp_path):
    """100 k contigs, about half reversed, a FASTA of more than 1 GiB (past the 256 MiB Infinity Cache, five chunks of
    PrintOutput's double buffer) == the numpy model on every byte"""
    asm = OU.seeded_assembly(100_000, 3000, 20000, 17)
    assert 0.45 < np.mean([d for s in asm['scaffolds'] for _, d, _, _ in s]) < 0.55
    want = OU.numpy_fasta(asm['scaffolds'], asm['pool'], asm['offsets'], asm['lengths'], asm['overlaps'], asm['sigma'], UID)
    assert want.shape[0] > 1 << 30
    param = OU.Param(200, asm['sigma'], str(tmp_path), io.StringIO())
    with OU.store_of(asm) as store:
        GO.PrintOutput(asm['F'], io.StringIO(), str(tmp_path), param, 1, store=store, unique_id=UID)
    path = str(tmp_path / 'pass1' / 'Scaffolds-pass1.fa')
    assert os.path.getsize(path) == want.shape[0]
    got = np.fromfile(path, dtype=np.uint8)
    os.remove(path)
    assert np.array_equal(got, want)
    merged = param.information_file.getvalue().splitlines()
    assert len(merged) > 100 and GO.last_timings['fasta_bytes'] == want.shape[0]


def test_cli_scaffolds_end_to_end(tmp_path):
    """FASTA + BAM on disk -> besst_amd.cli --scaffolds -y: every contig that was not set aside appears once, as it is
    or reverse-complemented, in exactly one scaffold"""
    from besst_amd import cli, synth
    from tests import bam_writer
    asm = synth.make_assembly(400, 1500, 7)
    batch = synth.simulate_library(asm, synth.LibrarySpec('fr', 500.0, 50.0), 30000, 8)
    rng = np.random.default_rng(9)
    seqs = {n: np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, int(l))].tobytes().decode()
            for n, l in zip(asm.names, asm.lengths)}
    fasta, bam = str(tmp_path / 'contigs.fa'), str(tmp_path / 'lib.bam')
    with open(fasta, 'w') as fh:
        for n, s in seqs.items():
            fh.write('>%s\n%s\n' % (n, s))
    bam_writer.write_bam(bam, batch)
    assert cli.main(['-c', fasta, '-f', bam, '-orientation', 'fr', '-o', str(tmp_path), '--scaffolds', '-y',
                     '-max_contig_overlap', '0']) == 0
    out = tmp_path / 'BESST_output'
    set_aside = set()
    for fname in ('repeats.fa', 'low_coverage_contigs.fa'):
        if (out / fname).exists():
            set_aside |= {l[1:].strip() for l in open(str(out / fname)) if l.startswith('>')}
    kept = [n for n in seqs if n not in set_aside]
    assert len(kept) > 300

    def canon(s):
        return min(s, OU.revcomp(s))

    lines = open(str(out / 'pass1' / 'Scaffolds-pass1.fa')).read().split('\n')
    assert lines[-1] == '' and all(l.startswith('>scaffold_') for l in lines[0:-1:2])
    bodies = lines[1:-1:2]
    pieces = [p for body in bodies for p in re.split('[Nn]+', body)]
    assert collections.Counter(canon(p) for p in pieces) == collections.Counter(canon(seqs[n]) for n in kept)
    stats = open(str(out / 'Statistics.txt')).read()
    assert int(re.search(r'\(super\)Contigs after scaffolding: (\d+)', stats).group(1)) == len(bodies)
    assert len(bodies) < len(kept)                                # something was joined
    rows = [l.split('\t') for l in open(str(out / 'pass1' / 'info-pass1.agp')) if not l.startswith('#')]
    assert sorted(r[5] for r in rows if r[4] == 'W') == sorted(kept)
    assert (out / 'pass1' / 'info-pass1.gff').exists() and (out / 'pass1' / 'edges_G.tsv').exists()
