"""Test-side restatement of the text the output stage writes next to the scaffold FASTA, from the rules and sharing nothing
with besst_amd.GenerateOutput:

  * ``agp_gff``: info-pass<n>.agp and info-pass<n>.gff of a list F (reference GenerateOutput.py:156-195, 208-221), pinned by
    the reference-captured text of tests/golden/scaffold_output.json.gz and tests/golden/flow_*.json.gz;
  * ``wrapped_fasta``: repeats.fa / low_coverage_contigs.fa (:47-53, 68-74), pinned by tests/golden/repeats_fasta.json.gz;
  * seeded layouts at the shapes where the device kernels can go wrong (tests/test_gpu_output_text.py).
"""
import gzip
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
REPEATS_GOLDEN = os.path.join(GOLDEN_DIR, 'repeats_fasta.json.gz')
AGP_HEADER = '##agp-version 2.0\n#lw-scaffolder output\n'
GFF_HEADER = '##gff-version 3\n'


def short_name(name):
    """The name up to, not including, its second '_'; the whole name if it has fewer than two."""
    first = name.find('_')
    second = name.find('_', first + 1) if first >= 0 else -1
    return name if second < 0 else name[:second]


def scaffold_lines(scaf, name):
    """-> (AGP lines, GFF lines) of one scaffold: tuples (contig, direction, position, length, ...) sorted by position"""
    agp, gff, comp, prev = [], [], 0, None
    for ctg, direction, pos, length in (t[:4] for t in scaf):
        sign = '+' if direction else '-'
        if prev is not None:
            gap = pos - (prev[0] + prev[1])
            if gap > 0:
                comp += 1
                lo = prev[0] + prev[1] + 1
                agp.append('%s\t%d\t%d\t%d\tN\t%d\tscaffold\tyes\tpaired-ends\n' % (name, lo, pos, comp, gap))
                gff.append('%s\tbesst_assembly\tgap\t%d\t%d\t.\t.\t.\t\n' % (name, lo, pos))
        comp += 1
        agp.append('%s\t%d\t%d\t%d\tW\t%s\t1\t%d\t%s\n' % (name, pos + 1, pos + length, comp, ctg, length, sign))
        gff.append('%s\tbesst_assembly\tcontig\t%d\t%d\t.\t%s\t.\tID=%s;Name=%s\n' % (name, pos + 1, pos + length, sign, ctg,
                                                                                 short_name(ctg)))
        prev = (pos, length)
    return agp, gff


def ordered(F):
    return [sorted(scaf, key=lambda t: t[2]) for scaf in reversed(F)]


def agp_gff(F, unique_id):
    """-> (AGP text, GFF text, lines per file without the headers)"""
    agp, gff = [AGP_HEADER], [GFF_HEADER]
    for k, scaf in enumerate(ordered(F)):
        a, g = scaffold_lines(scaf, 'scaffold_%d_uid_%d' % (k + 1, unique_id))
        agp += a
        gff += g
    return ''.join(agp), ''.join(gff), len(agp) - 1


def wrapped_fasta(records):
    """records: (name, sequence) -> '>' name, then lines of 60"""
    out = []
    for name, seq in records:
        out.append('>' + name + '\n')
        out.extend(seq[i:i + 60] + '\n' for i in range(0, len(seq), 60))
    return ''.join(out)


def load_repeats_golden():
    with gzip.open(REPEATS_GOLDEN, 'rt') as fh:
        return json.load(fh)


def F_of_state(state):
    """The list F that runBESST:205-216 / besst_amd.cli.write_scaffolds hand to PrintOutput, from the stored state of a
    pass of the flow fixtures: small scaffolds first, then the others, in dict order; no sequences."""
    ctg = {c[0]: c for c in state['contigs'] + state['small_contigs']}
    F = []
    for key in ('small_scaffolds', 'scaffolds'):
        for _key, _name, members, _length in state[key]:
            F.append([(m, bool(ctg[m][3]), ctg[m][2], ctg[m][4], '') for m in members])
    return F


class Param(object):
    """What PrintOutput reads of the parameter object, with the switch of the device text."""

    def __init__(self, out_dir=None, info=None, K=0, sigma=0.0, outputs_on_gpu=True):
        self.max_contig_overlap, self.std_dev_ins_size = K, sigma
        self.output_directory, self.information_file = out_dir, info
        self.outputs_on_gpu = outputs_on_gpu


# ---- seeded layouts ------------------------------------------------------------------------------------------------------
COORDS = [9, 10, 99, 100, 999, 1000, 9999, 10 ** 4, 10 ** 5 - 1, 10 ** 5, 10 ** 6 - 1, 10 ** 6, 10 ** 7 - 1, 10 ** 7,
          10 ** 8 - 1, 10 ** 8, 10 ** 9 - 1, 10 ** 9, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 10 ** 12, 2 ** 62 - 1]
NEGATIVE = [-1, -30, -10 ** 5]


def seeded_names(n, seed):
    """n distinct ASCII names: 1 and 300 bytes among them, 0, 1, 2 and 5 underscores, leading and doubled ones.  Their
    lengths vary from 1 up, so the names lie at odd offsets of the pool."""
    rng = np.random.default_rng(seed)
    shapes = ['%s', '_%s', '%s_', 'a_%s', 'a__%s', '_a_%s', '__%s', 'NODE_%s_length_7_cov_3', 'x_%s_y_z_w_v', '%s__', 'c%s',
              'q' * 280 + '_%s_tail']
    names = []
    for i in range(n):
        tag = str(i) + 'k' * int(rng.integers(0, 4))
        names.append(shapes[i % len(shapes)] % tag)
    if n > 3:
        names[1], names[2], names[3] = '_', 'Z', 'y' * 300
    assert len(set(names)) == n
    return names


def seeded_F(n_contigs, seed, boundaries=None, coords=False, names=None):
    """n contigs chained into scaffolds.  ``boundaries``: sorted flat indices at which a new scaffold starts (besides 0);
    None: seeded sizes of 1-6.  Gaps come from a menu around 0 (-1, 0, 1 among them), lengths include 0 and 1, some
    scaffolds start at a negative position; with ``coords`` the scaffolds start at the coordinates of COORDS / NEGATIVE and
    lengths are chosen so that starts and ends fall on both sides of the digit boundaries.
    -> (F as PrintOutput takes it - scaffolds last-first, tuples rotated -, names in output order)"""
    rng = np.random.default_rng(seed)
    names = seeded_names(n_contigs, seed) if names is None else names
    if boundaries is None:
        boundaries, at = [], 0
        while True:
            at += int(rng.integers(1, 7))
            if at >= n_contigs:
                break
            boundaries.append(at)
    starts = [0] + [b for b in boundaries if 0 < b < n_contigs]
    scaffolds = []
    gap_menu = (-1, 0, 1, -1, 0, 1, 2, 9, 10, 35, 99, 100, -7, 1000)
    len_menu = (0, 1, 1, 2, 9, 10, 11, 99, 100, 101, 1234, 99999)
    for k, lo in enumerate(starts):
        hi = starts[k + 1] if k + 1 < len(starts) else n_contigs
        if coords:
            pos = (COORDS + NEGATIVE)[k % (len(COORDS) + len(NEGATIVE))] - int(rng.integers(0, 2))
        else:
            pos = int(rng.choice((0, 0, 5, -1, -30, -10 ** 5, 12345)))
        scaf = []
        for i in range(lo, hi):
            length = int(len_menu[int(rng.integers(0, len(len_menu)))])
            if i > lo:
                pos += int(gap_menu[int(rng.integers(0, len(gap_menu)))])
            pos = min(pos, 2 ** 62 - 1)                          # (the device's range: magnitudes below 2^62)
            if pos + length >= 2 ** 62:
                length = 0
            scaf.append((names[i], bool(rng.integers(0, 2)), pos, length, ''))
            pos += length
        scaffolds.append(scaf)
    F = [scaf[1:] + scaf[:1] for scaf in reversed(scaffolds)]
    return F, names
