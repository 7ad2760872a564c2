#!/usr/bin/env python
"""Golden vectors for repeats.fa / low_coverage_contigs.fa: the reference's own GenerateOutput.PrintOutRepeats and
PrintOut_low_cowerage_contigs (BESST/GenerateOutput.py:47-58, 68-79), imported from the reference checkout through
tests/refharness and run on seeded contigs of lengths 0, 1, 59, 60, 61, 119, 120, 121, 180 and 200.

Stored: the contigs (name, sequence, which dict holds them), the order in which they are handed over, the text of the
two files and the keys left in Contigs / small_contigs afterwards.  Data only.

    python tests/golden/make_repeats_golden.py
"""
import gc
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

OUT = os.path.join(HERE, 'repeats_fasta.json.gz')
LENGTHS = (0, 1, 59, 60, 61, 119, 120, 121, 180, 200, 7, 60)
ALPHABET = 'ACGTNacgtnRYKM'


def contigs():
    """[name, sequence, 'Contigs' | 'small_contigs'] - names with and without underscores, one of 80 bytes"""
    rng = random.Random(20250117)
    out = []
    for i, n in enumerate(LENGTHS):
        name = ('ctg%d' % i, 'NODE_%d_length_%d_cov_5' % (i, n), '_%d_' % i, 'n' * 78 + '%02d' % i)[i % 4]
        out.append([name, ''.join(rng.choice(ALPHABET) for _ in range(n)), 'small_contigs' if i % 3 == 2 else 'Contigs'])
    return out


def orders(n):
    """the rows handed to the two writers: not in dict order"""
    return dict(repeats=[5, 0, 9, 2, 7, 11], low_coverage=[10, 1, 8, 3, 6, 4])


def run_reference(GO, mods, doc):
    out_dir = tempfile.mkdtemp(prefix='besst_rep_')
    try:
        objs = []
        dicts = dict(Contigs={}, small_contigs={})
        for name, seq, where in doc['contigs']:
            c = mods['Contig'].contig(name)
            c.sequence, c.length = seq, len(seq)
            objs.append(c)
            dicts[where][name] = c
        GO.PrintOutRepeats([objs[i] for i in doc['orders']['repeats']], dicts['Contigs'], out_dir, dicts['small_contigs'])
        GO.PrintOut_low_cowerage_contigs([objs[i] for i in doc['orders']['low_coverage']], dicts['Contigs'], out_dir,
                                         dicts['small_contigs'])
        gc.collect()                                             # the reference never closes its files
        expect = dict(left={k: list(v) for k, v in dicts.items()})
        for key, fname in (('repeats', 'repeats.fa'), ('low_coverage', 'low_coverage_contigs.fa')):
            with open(os.path.join(out_dir, fname), newline='') as fh:
                expect[key] = fh.read()
        return expect
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def load_reference():
    mods = loader.load()
    return importlib.import_module('BESST.GenerateOutput'), mods


def build():
    GO, mods = load_reference()
    doc = dict(generator='tests/golden/make_repeats_golden.py', contigs=contigs(), orders=orders(len(LENGTHS)))
    doc['expect'] = run_reference(GO, mods, doc)
    return doc


def main():
    doc = build()
    with gzip.GzipFile(OUT, 'wb', mtime=0) as gz, io.TextIOWrapper(gz, encoding='ascii') as fh:
        json.dump(doc, fh, separators=(',', ':'))
    print('wrote %s: %d contigs, %.1f KB' % (OUT, len(doc['contigs']), os.path.getsize(OUT) / 1024.0))


if __name__ == '__main__':
    main()
