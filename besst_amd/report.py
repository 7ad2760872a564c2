"""The BAM report: what a resident BAM holds, counted over all of its records in one pass on the GPU (csrc/report.hip;
besst_dev_library_report / besst_ctx_library_report, the word layout in include/besst_amd.h).

``LibraryReport`` names the words: the flag census (samtools flagstat's sixteen rows, QC-pass and QC-fail), the counts per
reference (samtools idxstats' numbers), the mapq and aligned-length histograms, the pairs on one reference by class with
their |tlen| histograms, and a two-word digest of the columns.  Every word is a sum over the records (the digest's second an
xor), so the reports of the slices of a stream add up: ``a + b``.  ``write`` / ``read`` keep a report as TSV files.
"""
import os

import numpy as np

from . import _lib

CENSUS_LABELS = ('in total', 'primary', 'secondary', 'supplementary', 'duplicates', 'primary duplicates', 'mapped',
                 'primary mapped', 'paired in sequencing', 'read1', 'read2', 'properly paired',
                 'with itself and mate mapped', 'singletons', 'with mate mapped to a different chr',
                 'with mate mapped to a different chr (mapQ>=5)')
PAIR_CLASSES = ('innie', 'outie', 'tandem', 'other')
DEFAULT_ISIZE_BINS = 32768
MAX_ISIZE_BINS = 1 << 20
# word offsets (include/besst_amd.h, BESST_REPORT_*)
CENSUS, UNPLACED, TID_OUT_OF_RANGE, PAIRS, DIGEST_SUM, DIGEST_XOR, MAPQ, QLEN, REFS = 0, 32, 33, 34, 38, 39, 40, 296, 65832
FILES = ('bam_report.tsv', 'idxstats.tsv', 'mapq_hist.tsv', 'qlen_hist.tsv', 'insert_sizes.tsv')


def report_words(n_refs, isize_bins):
    """Length of a report in 64-bit words (besst_dev_library_report_words)."""
    if not 0 <= n_refs < 1 << 31 or not 1 <= isize_bins <= MAX_ISIZE_BINS:
        raise ValueError('report: n_refs must lie in 0 .. 2^31-1 and isize_bins in 1 .. 2^20')
    return REFS + 2 * int(n_refs) + 3 * (int(isize_bins) + 1)


class LibraryReport(object):
    """Named views over the words of a report.  ``references`` / ``lengths``: the header's, when the maker knew them
    (idxstats.tsv names its rows with them)."""

    def __init__(self, words, n_refs, isize_bins=DEFAULT_ISIZE_BINS, references=None, lengths=None):
        self.n_refs, self.isize_bins = int(n_refs), int(isize_bins)
        w = np.ascontiguousarray(words).view(np.uint64).reshape(-1)
        if w.shape[0] != report_words(self.n_refs, self.isize_bins):
            raise ValueError('report: %d words do not fit n_refs=%d, isize_bins=%d' % (w.shape[0], self.n_refs, self.isize_bins))
        self.words = w
        self.references = list(references) if references is not None else None
        self.lengths = [int(x) for x in lengths] if lengths is not None else None
        c = w.view(np.int64)
        self.census = c[CENSUS:CENSUS + 32].reshape(16, 2)             # [row, 0 QC-pass | 1 QC-fail]
        self.pair_classes = c[PAIRS:PAIRS + 4]                         # innie, outie, tandem, other
        self.mapq = c[MAPQ:MAPQ + 256]
        self.qlen = c[QLEN:QLEN + 65536]
        self.mapped = c[REFS:REFS + self.n_refs]
        self.placed_unmapped = c[REFS + self.n_refs:REFS + 2 * self.n_refs]
        h = REFS + 2 * self.n_refs
        k = self.isize_bins + 1
        self.innie, self.outie, self.tandem = c[h:h + k], c[h + k:h + 2 * k], c[h + 2 * k:h + 3 * k]

    unplaced = property(lambda self: int(self.words[UNPLACED]))
    tid_out_of_range = property(lambda self: int(self.words[TID_OUT_OF_RANGE]))
    digest = property(lambda self: (int(self.words[DIGEST_SUM]), int(self.words[DIGEST_XOR])))
    n_records = property(lambda self: int(self.census[0].sum()))

    def census_rows(self):
        """[(label, QC-pass, QC-fail)] in samtools flagstat's order."""
        return [(lab, int(self.census[r, 0]), int(self.census[r, 1])) for r, lab in enumerate(CENSUS_LABELS)]

    def __add__(self, other):
        if not isinstance(other, LibraryReport):
            return NotImplemented
        if (self.n_refs, self.isize_bins) != (other.n_refs, other.isize_bins):
            raise ValueError('reports of different shapes do not add')
        words = self.words + other.words                               # (uint64: the digest's sum wraps, as it should)
        words[DIGEST_XOR] = self.words[DIGEST_XOR] ^ other.words[DIGEST_XOR]
        return LibraryReport(words, self.n_refs, self.isize_bins, self.references or other.references,
                             self.lengths or other.lengths)

    def __eq__(self, other):
        return (isinstance(other, LibraryReport) and (self.n_refs, self.isize_bins) == (other.n_refs, other.isize_bins)
                and bool(np.array_equal(self.words, other.words)))

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def census_lines(self):
        """The sixteen rows as text, the way samtools flagstat words them."""
        return ['%d + %d %s' % (p, f, lab) for lab, p, f in self.census_rows()]

    # ---- files ---------------------------------------------------------------------------------------------------
    def write(self, directory):
        """bam_report.tsv, idxstats.tsv, mapq_hist.tsv, qlen_hist.tsv, insert_sizes.tsv into ``directory``."""
        os.makedirs(directory, exist_ok=True)
        with open(os.path.join(directory, 'bam_report.tsv'), 'w') as fh:
            fh.write('label\tpass\tfail\n')
            for lab, p, f in self.census_rows():
                fh.write('%s\t%d\t%d\n' % (lab, p, f))
            fh.write('unplaced\t%d\n' % self.unplaced)
            fh.write('tid_out_of_range\t%d\n' % self.tid_out_of_range)
            for name, v in zip(PAIR_CLASSES, self.pair_classes.tolist()):
                fh.write('pairs %s\t%d\n' % (name, v))
            fh.write('n_refs\t%d\n' % self.n_refs)
            fh.write('isize_bins\t%d\n' % self.isize_bins)
            fh.write('digest_sum\t0x%016x\n' % self.digest[0])
            fh.write('digest_xor\t0x%016x\n' % self.digest[1])
        names = self.references if self.references is not None else [str(i) for i in range(self.n_refs)]
        lengths = self.lengths if self.lengths is not None else [0] * self.n_refs
        with open(os.path.join(directory, 'idxstats.tsv'), 'w') as fh:
            fh.write('name\tlength\tmapped\tplaced_unmapped\n')
            fh.write(''.join('%s\t%d\t%d\t%d\n' % row for row in
                             zip(names, lengths, self.mapped.tolist(), self.placed_unmapped.tolist())))
            fh.write('*\t0\t0\t%d\n' % self.unplaced)
        for fname, col, hist in (('mapq_hist.tsv', 'mapq', self.mapq), ('qlen_hist.tsv', 'qlen', self.qlen)):
            with open(os.path.join(directory, fname), 'w') as fh:
                fh.write('%s\tcount\n' % col)
                for v in np.flatnonzero(hist).tolist():
                    fh.write('%d\t%d\n' % (v, hist[v]))
        with open(os.path.join(directory, 'insert_sizes.tsv'), 'w') as fh:
            fh.write('|tlen|\tinnie\toutie\ttandem\n')
            b = self.isize_bins
            for v in np.flatnonzero(self.innie[:b] | self.outie[:b] | self.tandem[:b]).tolist():
                fh.write('%d\t%d\t%d\t%d\n' % (v, self.innie[v], self.outie[v], self.tandem[v]))
            fh.write('>=%d\t%d\t%d\t%d\n' % (b, self.innie[b], self.outie[b], self.tandem[b]))

    @classmethod
    def read(cls, directory):
        """The report that ``write`` left in ``directory``."""
        def rows(fname):
            with open(os.path.join(directory, fname)) as fh:
                return [line.rstrip('\n').split('\t') for line in fh][1:]
        top = rows('bam_report.tsv')
        scalars = {r[0]: r[1] for r in top[16:]}
        n_refs, bins = int(scalars['n_refs']), int(scalars['isize_bins'])
        w = np.zeros(report_words(n_refs, bins), dtype=np.uint64)
        c = w.view(np.int64)
        for r, (lab, p, f) in enumerate(top[:16]):
            if lab != CENSUS_LABELS[r]:
                raise ValueError('bam_report.tsv: row %d is %r, not %r' % (r, lab, CENSUS_LABELS[r]))
            c[CENSUS + 2 * r], c[CENSUS + 2 * r + 1] = int(p), int(f)
        c[UNPLACED], c[TID_OUT_OF_RANGE] = int(scalars['unplaced']), int(scalars['tid_out_of_range'])
        for k, name in enumerate(PAIR_CLASSES):
            c[PAIRS + k] = int(scalars['pairs ' + name])
        w[DIGEST_SUM], w[DIGEST_XOR] = int(scalars['digest_sum'], 16), int(scalars['digest_xor'], 16)
        idx = rows('idxstats.tsv')
        if len(idx) != n_refs + 1 or idx[-1][0] != '*' or int(idx[-1][3]) != int(scalars['unplaced']):
            raise ValueError('idxstats.tsv does not match bam_report.tsv')
        names, lengths = [r[0] for r in idx[:-1]], [int(r[1]) for r in idx[:-1]]
        for i, r in enumerate(idx[:-1]):
            c[REFS + i], c[REFS + n_refs + i] = int(r[2]), int(r[3])
        for fname, base in (('mapq_hist.tsv', MAPQ), ('qlen_hist.tsv', QLEN)):
            for v, n in rows(fname):
                c[base + int(v)] = int(n)
        h = REFS + 2 * n_refs
        for r in rows('insert_sizes.tsv'):
            v = bins if r[0].startswith('>=') else int(r[0])
            for k in range(3):
                c[h + k * (bins + 1) + v] = int(r[1 + k])
        return cls(w, n_refs, bins, names, lengths)


def orientation_note(report, named):
    """A sentence when the pairs on one reference speak against the orientation the library was named with: the class
    that belongs to ``named`` ('fr': innie, 'rf': outie) holds under 10 % of innie + outie, of at least 1000 such pairs;
    else None.  The 10 % is low on purpose: the same-contig pairs of a mate-pair library on a fragmented assembly are
    mostly its paired-end contamination, and a majority rule would accuse correct 'rf' runs."""
    if named not in ('fr', 'rf'):
        raise ValueError("orientation must be 'fr' or 'rf'")
    innie, outie = int(report.pair_classes[0]), int(report.pair_classes[1])
    total = innie + outie
    mine = innie if named == 'fr' else outie
    if total < 1000 or mine * 10 >= total:
        return None
    kind, other = ('innie', 'rf') if named == 'fr' else ('outie', 'fr')
    return ("NOTE: the library is named -orientation %s, but only %d of the %d pairs that lie on one contig with opposite "
            "strands (%.1f %%) are %s pairs; was it meant to be %s?" % (named, mine, total, 100.0 * mine / total, kind, other))


def length_mismatches(references, lengths, contig_lengths):
    """Contigs whose length in the FASTA (``contig_lengths``: name -> length) differs from the BAM header's @SQ length ->
    [(name, header length, FASTA length)] in header order; a BAM mapped to another contig file shows here."""
    return [(name, int(hl), int(contig_lengths[name])) for name, hl in zip(references, lengths)
            if name in contig_lengths and int(contig_lengths[name]) != int(hl)]


def dev_report_tensor(rec, n_refs, isize_bins=DEFAULT_ISIZE_BINS, tid_bits=None):
    """besst_dev_library_report over torch-owned device columns (pipeline.DeviceRecords, or anything with its eight column
    attributes and ``n``) on torch's current stream -> the words as a device tensor of int64 (bit patterns of uint64)."""
    import ctypes as C
    import torch
    lib = _lib.load()
    words = report_words(n_refs, isize_bins)
    dev = rec.tid.device
    out = torch.empty(words, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None and rec.n else None
    args = _lib.ReportArgs(p(rec.tid), p(rec.mtid), p(rec.pos), p(rec.mpos), p(rec.tlen), p(rec.flag), p(rec.mapq),
                           p(rec.qlen), p(tid_bits), int(rec.n), int(n_refs), int(isize_bins), words)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.besst_dev_library_report(C.c_void_p(stream), C.byref(args), C.c_void_p(out.data_ptr())),
                   'dev_library_report')
    return out
