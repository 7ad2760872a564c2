#!/usr/bin/env python
"""Golden vectors for the scaffold output stage: the reference's own GenerateOutput.PrintOutput
(BESST/GenerateOutput.py:197-227 with the Scaffold class of :105-195), imported from the reference checkout through
tests/refharness with time.time pinned, run on seeded lists F.

Stored per case: the inputs (F, max_contig_overlap K, std_dev_ins_size sigma) and what the call left behind - the text of
Scaffolds-pass1.fa, info-pass1.agp and info-pass1.gff, what it printed to Information, the `merging` lines it printed to
param.information_file, and - where it raised - the KeyError's character (the files are then not stored: they are
whatever had been flushed).  Once per file: rev_nuc as a 256-entry table.  Data only.

Case groups: planted overlaps of 1, 19, 20, 21, K-1, K, K+1 and whole-contig length for K in {0, 1, 64, 200}; gaps of
-30, -1, 0, 1, 2, int(2 sigma), int(2 sigma)+1, 500 with sigma 50, 12.7 and 0, with and without a planted overlap;
contigs shorter than K and of length 1 and 2, the whole IUPAC alphabet in both cases, single-contig scaffolds, tuples
handed over unsorted and with equal positions; contigs holding 'U' or 'x', reversed (KeyError) and forward (none); a
seeded mix of longer scaffolds.

    python tests/golden/make_output_golden.py
"""
import gzip
import importlib
import io
import json
import os
import random
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests.refharness import loader  # noqa: E402

OUT = os.path.join(HERE, 'scaffold_output.json.gz')
UNIQUE_ID = 1700000000
ALPHABET = 'ACGTNXYRKMSWBVHD' + 'acgtnyrkmswbvhd'
_COMP = dict(zip('ACGT', 'TGCA'))


def rand_seq(rng, n, alphabet='ACGT'):
    return ''.join(rng.choice(alphabet) for _ in range(n))


def rc(s):
    return ''.join(_COMP[c] for c in reversed(s))


def stored(oriented_seq, direction):
    """The sequence to store so that the contig, written in `direction`, reads `oriented_seq` (ACGT only)."""
    return oriented_seq if direction else rc(oriented_seq)


def pair_with_overlap(rng, ov, len_a, len_b, dir_a, dir_b, gap, tag):
    """Two contigs whose oriented ends share exactly `ov` planted bases (ov <= both lengths)."""
    a = rand_seq(rng, len_a)
    shared = a[len_a - ov:] if ov else ''
    # the base after the shared stretch differs from what would extend a longer match by accident only rarely; the
    # reference decides, the fixture records
    b = shared + rand_seq(rng, len_b - ov)
    return [(tag + '_a', dir_a, 0, len_a, stored(a, dir_a)), (tag + '_b', dir_b, len_a + gap, len_b, stored(b, dir_b))]


def overlap_cases(rng):
    out = []
    for K in (0, 1, 64, 200):
        F = []
        wanted = sorted({1, 19, 20, 21, max(K - 1, 0), K, K + 1})
        for n, ov in enumerate(wanted):
            for d, (da, db) in enumerate(((True, True), (True, False), (False, True), (False, False))):
                F.append(pair_with_overlap(rng, ov, 260 + 7 * n, 300 + 5 * d, da, db, 0, 'K%d_ov%d_%d' % (K, ov, d)))
        # whole-contig length: the right contig is nothing but the shared stretch, and the left one likewise
        for L in (25, 64, 200, 230):
            whole = rand_seq(rng, L)
            F.append([('K%d_whole%d_a' % (K, L), True, 0, 400, rand_seq(rng, 400 - L) + whole),
                      ('K%d_whole%d_b' % (K, L), False, 400, L, rc(whole))])
            F.append([('K%d_both%d_a' % (K, L), False, 0, L, rc(whole)), ('K%d_both%d_b' % (K, L), True, L, L, whole)])
        out.append(dict(name='overlaps_K%d' % K, K=K, sigma=50.0, F=F))
    return out


def gap_cases(rng):
    out = []
    for sigma in (50.0, 12.7, 0, 0.4):
        F = []
        edge = int(2 * sigma)
        for gap in (-30, -1, 0, 1, 2, edge, edge + 1, 500):
            for ov in (0, 30):
                for da, db in ((True, True), (False, False), (True, False)):
                    F.append(pair_with_overlap(rng, ov, 90, 120, da, db, gap, 's%s_g%d_o%d_%d%d' % (sigma, gap, ov, da, db)))
        out.append(dict(name='gaps_sigma%s' % sigma, K=200, sigma=sigma, F=F))
    return out


def short_cases(rng):
    F = []
    for L in (1, 2, 3, 19, 20, 21):
        F.append([('single_%d' % L, L % 2 == 0, 0, L, rand_seq(rng, L, ALPHABET))])
        F.append([('tiny%d_a' % L, True, 0, L, rand_seq(rng, L)), ('tiny%d_b' % L, False, L, L, rand_seq(rng, L)),
                  ('tiny%d_c' % L, False, 2 * L + 3, 1, rand_seq(rng, 1, ALPHABET))])
    # the whole alphabet, both directions, next to each other
    F.append([('iupac_fwd', True, 0, len(ALPHABET), ALPHABET), ('iupac_rev', False, len(ALPHABET) + 5, len(ALPHABET), ALPHABET),
              ('iupac_long', False, 100, 150, rand_seq(rng, 150, ALPHABET))])
    # homopolymers: every length matches
    F.append([('poly_a', True, 0, 50, 'A' * 50), ('poly_b', True, 50, 30, 'A' * 30), ('poly_c', False, 80, 70, 'T' * 70)])
    # case matters: the same letters in the other case do not match
    shared = rand_seq(rng, 40)
    F.append([('case_a', True, 0, 100, rand_seq(rng, 60) + shared), ('case_b', True, 100, 90, shared.lower() + rand_seq(rng, 50))])
    # handed over unsorted, and with equal positions (the sort is stable)
    F.append([('uns_c', True, 700, 80, rand_seq(rng, 80)), ('uns_a', False, 0, 300, rand_seq(rng, 300)),
              ('uns_b', True, 310, 380, rand_seq(rng, 380)), ('uns_d', False, 700, 60, rand_seq(rng, 60)),
              ('uns_e', True, 310, 5, rand_seq(rng, 5))])
    # lengths in the tuple that differ from the sequence's: positions and gaps follow the tuple
    F.append([('len_a', True, 0, 100, rand_seq(rng, 90)), ('len_b', False, 120, 50, rand_seq(rng, 75))])
    return [dict(name='short_K200', K=200, sigma=30.0, F=F), dict(name='short_K5', K=5, sigma=30.0, F=F)]


def keyerror_cases(rng):
    out = []
    merged = pair_with_overlap(rng, 40, 150, 150, True, False, 0, 'ok')
    for ch in ('U', 'x'):
        bad = rand_seq(rng, 50) + ch + rand_seq(rng, 30) + ch.lower() + rand_seq(rng, 20)
        out.append(dict(name='forward_%s' % ch, K=200, sigma=50.0,
                        F=[[('fwd_%s' % ch, True, 0, len(bad), bad), ('after', False, 200, 60, rand_seq(rng, 60))]]))
        # reversed: the first scaffold written (the last of F) merges, the second holds the byte
        out.append(dict(name='reversed_%s' % ch, K=200, sigma=50.0,
                        F=[[('never', False, 0, 40, rand_seq(rng, 40))],
                           [('good', True, 0, 80, rand_seq(rng, 80)), ('rev_%s' % ch, False, 90, len(bad), bad)],
                           merged]))
        out.append(dict(name='reversed_first_%s' % ch, K=200, sigma=50.0,
                        F=[[('rev1_%s' % ch, False, 0, len(bad), bad), ('tail', True, 150, 30, rand_seq(rng, 30))]]))
    # the byte lies in the stretch a merge would drop: the reference still trips over it
    a = rand_seq(rng, 120)
    b_oriented = a[-30:] + rand_seq(rng, 90)
    b_stored = rc(b_oriented)
    b_stored = b_stored[:-10] + 'U' + b_stored[-9:]               # oriented position 9, inside the 30 shared bases
    out.append(dict(name='reversed_in_overlap', K=200, sigma=50.0,
                    F=[[('ov_a', True, 0, 120, a), ('ov_b', False, 120, 120, b_stored)], merged]))
    # a candidate junction whose LEFT contig is reversed and bad: it failed when it was written
    out.append(dict(name='reversed_left', K=64, sigma=10.0,
                    F=[[('l_a', True, 0, 50, rand_seq(rng, 50)), ('l_b', False, 50, 70, rand_seq(rng, 35) + '*' + rand_seq(rng, 34)),
                        ('l_c', False, 120, 70, rand_seq(rng, 69) + '-')]]))
    # not a candidate (gap above 2 sigma): found when the contig is written
    out.append(dict(name='reversed_far', K=200, sigma=1.0,
                    F=[[('f_a', True, 0, 50, rand_seq(rng, 50)), ('f_b', False, 500, 40, rand_seq(rng, 20) + 'u' + rand_seq(rng, 19))]]))
    return out


def mixed_case(rng):
    F = []
    n = 0
    for s in range(30):
        scaf, pos, prev_oriented = [], 0, None
        for c in range(rng.choice((1, 2, 3, 5, 9))):
            length = rng.choice((15, 40, 180, 333, 700, 1500))
            direction = rng.random() < 0.5
            alphabet = 'ACGT' if rng.random() < 0.8 else 'ACGTacgtNnRYKM'
            seq_o = rand_seq(rng, length, alphabet)
            gap = rng.choice((-5, 0, 0, 1, 2, 35, 99, 100, 101, 250))
            if prev_oriented is not None and rng.random() < 0.4 and alphabet == 'ACGT':
                ov = min(rng.choice((12, 20, 25, 60, 150, 199, 200, 210)), length, len(prev_oriented))
                if all(ch in _COMP for ch in prev_oriented[-ov:]):
                    seq_o = prev_oriented[-ov:] + seq_o[ov:]
            if prev_oriented is not None:
                pos += gap
            seq_s = seq_o if direction else ''.join(
                {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A', 'a': 't', 'c': 'g', 'g': 'c', 't': 'a', 'N': 'N', 'n': 'n', 'R': 'Y',
                 'Y': 'R', 'K': 'M', 'M': 'K'}[ch] for ch in reversed(seq_o))
            scaf.append(('NODE_%d_length_%d_cov_%d' % (n, length, rng.randint(3, 90)), direction, pos, length, seq_s))
            n += 1
            pos += length
            prev_oriented = seq_o
        rng.shuffle(scaf)
        F.append(scaf)
    return [dict(name='mixed', K=200, sigma=50.0, F=F)]


def all_cases():
    rng = random.Random(20240929)
    return overlap_cases(rng) + gap_cases(rng) + short_cases(rng) + keyerror_cases(rng) + mixed_case(rng)


def run_reference(GO, mods, case):
    """One PrintOutput call of the real reference on the case's inputs -> the `expect` document."""
    out_dir = tempfile.mkdtemp(prefix='besst_out_')
    try:
        param = mods['Parameter'].parameter()
        param.max_contig_overlap = case['K']
        param.std_dev_ins_size = case['sigma']
        param.output_directory = out_dir
        param.information_file = io.StringIO()
        info = io.StringIO()
        F = [[(n, bool(d), p, l, s) for n, d, p, l, s in scaf] for scaf in case['F']]
        key_error = None
        try:
            GO.PrintOutput(F, info, out_dir, param, 1)
        except KeyError as exc:
            key_error = exc.args[0]
        expect = dict(information=info.getvalue(), merging=param.information_file.getvalue().splitlines(),
                      key_error=key_error, fasta=None, agp=None, gff=None)
        if key_error is None:
            import gc
            gc.collect()                                         # the reference never closes its three files
            for key, fname in (('fasta', 'Scaffolds-pass1.fa'), ('agp', 'info-pass1.agp'), ('gff', 'info-pass1.gff')):
                with open(os.path.join(out_dir, 'pass1', fname)) as fh:
                    expect[key] = fh.read()
        return expect
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def load_reference():
    mods = loader.load()
    GO = importlib.import_module('BESST.GenerateOutput')
    GO.time.time = lambda: float(UNIQUE_ID)                      # (GenerateOutput's `time` is the module)
    return GO, mods


def rev_nuc_table(GO):
    tab = [0] * 256
    for k, v in GO.rev_nuc.items():
        tab[ord(k)] = ord(v)
    return tab


def build():
    GO, mods = load_reference()
    cases = []
    for case in all_cases():
        doc = dict(name=case['name'], K=case['K'], sigma=case['sigma'],
                   F=[[list(t) for t in scaf] for scaf in case['F']])
        doc['expect'] = run_reference(GO, mods, doc)
        cases.append(doc)
    return dict(generator='tests/golden/make_output_golden.py', unique_id=UNIQUE_ID, rev_nuc=rev_nuc_table(GO), cases=cases)


def main():
    doc = build()
    with gzip.GzipFile(OUT, 'wb', mtime=0) as gz, io.TextIOWrapper(gz, encoding='ascii') as fh:
        json.dump(doc, fh, separators=(',', ':'))
    cases = doc['cases']
    print('wrote %s: %d cases, %d contigs, %d merges, %d KeyErrors, %.1f KB' % (
        OUT, len(cases), sum(len(s) for c in cases for s in c['F']), sum(len(c['expect']['merging']) for c in cases),
        sum(1 for c in cases if c['expect']['key_error'] is not None), os.path.getsize(OUT) / 1024.0))


if __name__ == '__main__':
    main()
