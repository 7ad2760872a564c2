"""The assembly report: what the contigs and every pass's scaffolds hold, counted on the GPU where the bytes lie.

The census of a byte string is 16 words of int64 (include/besst_amd.h, BESST_CENSUS_*): bases by class, lower case, and
the runs of 'N'.  csrc/seq_census.hip counts it for every row of a segment table over a window of a byte stream and
merges the windows of a stream in order, so the contig pool of a ``SequenceStore`` is one call (:func:`census_store`) and
any ``ByteSource`` - the scaffold FASTA of a pass as ``ScaffoldEmitter`` produces it - is a walk over windows of one scratch
buffer (:func:`census_source`).  :class:`SequenceCensus` names the columns and keeps the table as TSV;
:class:`AssemblyStats` is the summary an assembly-statistics tool prints (Nx / Lx, auN, GC, gaps), made from a census in
numpy on the host.  ``PrintOutput`` writes both per pass when ``param.assembly_report`` is set (:func:`write_pass_report`),
the command line with ``--assembly_report``.
"""
from __future__ import print_function

import ctypes as _C

import numpy as np

from . import _lib
from ._lib import BesstDeviceError

WORDS = 16                                # include/besst_amd.h: BESST_CENSUS_WORDS
(LEN, A, C, G, T, N, IUPAC, OTHER, LOWER, PRE, SUF, RUNS, GAPS, GAP_BASES, LONGEST) = range(15)
COLUMNS = ('name', 'length', 'A', 'C', 'G', 'T', 'N', 'iupac', 'other', 'lower', 'gc', 'n_runs', 'gaps', 'gap_bases',
           'longest_gap')
_WORD_OF = dict(length=LEN, A=A, C=C, G=G, T=T, N=N, iupac=IUPAC, other=OTHER, lower=LOWER, n_runs=RUNS, gaps=GAPS,
                gap_bases=GAP_BASES, longest_gap=LONGEST)


class SequenceCensus(object):
    """``names`` and the ``n_seq x 16`` census words of as many sequences.  The words as the device leaves them are
    PARTIAL: the runs of 'N' at either end of a sequence are open (``pre`` / ``suf``).  ``finalised()`` closes them into
    ``n_runs`` / ``gaps`` / ``gap_bases`` / ``longest_gap`` (a run counts as a gap from ``min_gap`` bases on); the named
    columns are views of whichever form the object holds."""

    def __init__(self, names, words, min_gap=1, final=False):
        self.names = list(names)
        self.words = np.ascontiguousarray(words, dtype=np.int64).reshape(-1, WORDS)
        if len(self.names) != len(self.words):
            raise ValueError('need one name per census row')
        self.min_gap, self.final = int(min_gap), bool(final)

    def __len__(self):
        return len(self.names)

    def __getattr__(self, column):
        if column in _WORD_OF:
            return self.words[:, _WORD_OF[column]]
        if column in ('pre', 'suf'):
            return self.words[:, PRE if column == 'pre' else SUF]
        raise AttributeError(column)

    @property
    def gc(self):
        """(G + C) / (A + C + G + T) per sequence; nan where the denominator is 0"""
        w = self.words
        acgt = w[:, A] + w[:, C] + w[:, G] + w[:, T]
        out = np.full(len(w), np.nan)
        np.divide(w[:, G] + w[:, C], acgt, out=out, where=acgt > 0)
        return out

    def finalised(self):
        if self.final:
            return self
        w = self.words.copy()
        all_n = (w[:, LEN] > 0) & (w[:, PRE] == w[:, LEN])
        for mask, column in ((all_n, LEN), (~all_n & (w[:, PRE] > 0), PRE), (~all_n & (w[:, SUF] > 0), SUF)):
            length = w[:, column].copy()
            w[mask, RUNS] += 1
            gap = mask & (length >= self.min_gap)
            w[gap, GAPS] += 1
            w[gap, GAP_BASES] += length[gap]
            w[mask, LONGEST] = np.maximum(w[mask, LONGEST], length[mask])
        w[:, PRE] = w[:, SUF] = 0
        return SequenceCensus(self.names, w, self.min_gap, True)

    def select(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        return SequenceCensus([self.names[r] for r in rows.tolist()], self.words[rows], self.min_gap, self.final)

    def write(self, path):
        """The finalised table as TSV, one row per sequence (``#min_gap`` in the first line; ``gc`` with six decimals,
        empty where there is no A, C, G or T)."""
        c = self.finalised()
        gc = c.gc
        with open(path, 'w') as fh:
            print('#min_gap=%d' % c.min_gap, file=fh)
            print('\t'.join(COLUMNS), file=fh)
            for i, name in enumerate(c.names):
                row = [str(name)]
                for column in COLUMNS[1:]:
                    if column == 'gc':
                        row.append('' if np.isnan(gc[i]) else '%.6f' % gc[i])
                    else:
                        row.append(str(int(c.words[i, _WORD_OF[column]])))
                print('\t'.join(row), file=fh)

    @classmethod
    def read(cls, path):
        """What ``write`` left: the finalised census (names as strings)."""
        names, rows, min_gap = [], [], 1
        with open(path) as fh:
            first = fh.readline().rstrip('\n')
            if first.startswith('#min_gap='):
                min_gap = int(first.split('=', 1)[1])
                first = fh.readline().rstrip('\n')
            if tuple(first.split('\t')) != COLUMNS:
                raise ValueError('%s: not a sequence report (columns %r)' % (path, first))
            for line in fh:
                f = line.rstrip('\n').split('\t')
                if len(f) != len(COLUMNS):
                    raise ValueError('%s: a row of %d fields' % (path, len(f)))
                names.append(f[0])
                w = [0] * WORDS
                for column, value in zip(COLUMNS[1:], f[1:]):
                    if column != 'gc':
                        w[_WORD_OF[column]] = int(value)
                rows.append(w)
        return cls(names, np.asarray(rows, dtype=np.int64).reshape(-1, WORDS), min_gap, True)


class AssemblyStats(object):
    """The summary of a census: ``n`` sequences, ``total`` / ``min`` / ``max`` / ``mean`` length, Nx and Lx, auN, GC, the
    bases by class, gaps, and the sequences of at least 1 000 and 10 000 bases.  Integers are exact."""

    def __init__(self, census):
        c = census.finalised()
        lengths = c.words[:, LEN]
        self._desc = np.sort(lengths)[::-1]
        self._cum = np.cumsum(self._desc)
        self.n = int(len(lengths))
        self.total = int(lengths.sum())
        self.min = int(lengths.min()) if self.n else 0
        self.max = int(lengths.max()) if self.n else 0
        self.mean = self.total / float(self.n) if self.n else 0.0
        self.auN = float((lengths.astype(np.float64) ** 2).sum() / self.total) if self.total else 0.0
        s = c.words.sum(axis=0) if self.n else np.zeros(WORDS, dtype=np.int64)
        acgt = int(s[A] + s[C] + s[G] + s[T])
        self.gc = (int(s[G]) + int(s[C])) / float(acgt) if acgt else None
        self.n_bases, self.iupac_bases, self.other_bases = int(s[N]), int(s[IUPAC]), int(s[OTHER])
        self.lower_bases = int(s[LOWER])
        self.n_runs, self.gaps, self.gap_bases = int(s[RUNS]), int(s[GAPS]), int(s[GAP_BASES])
        self.longest_gap = int(c.words[:, LONGEST].max()) if self.n else 0
        self.sequences_with_other = int((c.words[:, OTHER] > 0).sum())
        self.n_1k, self.bases_1k = int((lengths >= 1000).sum()), int(lengths[lengths >= 1000].sum())
        self.n_10k, self.bases_10k = int((lengths >= 10000).sum()), int(lengths[lengths >= 10000].sum())
        self.N50, self.L50, self.N90, self.L90 = self.nx(50), self.lx(50), self.nx(90), self.lx(90)

    def _reached(self, x):
        """index into the descending lengths of the first one where cumsum * 100 >= x * total (None: no sequence)"""
        if not self.n:
            return None
        x = int(x)
        if x != float(x) or not 0 <= x <= 100:
            raise ValueError('x must be a whole number in 0..100')
        return int(np.searchsorted(self._cum * 100, x * self.total, side='left'))

    def nx(self, x):
        """The length at which the descending lengths have reached x percent of the total; None without sequences."""
        at = self._reached(x)
        return None if at is None else int(self._desc[at])

    def lx(self, x):
        """How many of the longest sequences it takes to reach x percent of the total; 0 without sequences."""
        at = self._reached(x)
        return 0 if at is None else at + 1

    def rows(self):
        """(metric, value) in the order of assembly_stats.tsv"""
        return [(k, getattr(self, k)) for k in (
            'n', 'total', 'min', 'max', 'mean', 'N50', 'L50', 'N90', 'L90', 'auN', 'gc', 'n_bases', 'n_runs', 'gaps',
            'gap_bases', 'longest_gap', 'lower_bases', 'iupac_bases', 'other_bases', 'sequences_with_other', 'n_1k',
            'bases_1k', 'n_10k', 'bases_10k')]


def reference_n60(lengths):
    """``decide_approach.NX(60, lengths)`` of the reference, float expression and all: the first of the descending lengths
    at which the running sum reaches ``total / (100 / 60.0)``.  None for no lengths.  runBESST switches to path finding
    where this is below the library's ``ins_size_threshold`` and path extension is on."""
    desc = sorted((int(v) for v in lengths), reverse=True)
    stop = sum(desc) / (100 / float(60))
    running = 0
    for length in desc:
        running += length
        if running >= stop:
            return length
    return None


def _fmt(value):
    if value is None:
        return ''
    if isinstance(value, float):
        return '%.6f' % value
    return str(value)


def check_table(seq_off, seq_len):
    """ValueError naming the first row of a segment table that is out of order or overlaps its predecessor."""
    off, length = np.asarray(seq_off, dtype=np.int64), np.asarray(seq_len, dtype=np.int64)
    if off.shape != length.shape or off.ndim != 1:
        raise ValueError('seq_off and seq_len must be two columns of one length')
    bad = (off < 0) | (length < 0)
    if len(off) > 1:
        bad[1:] |= off[1:] < off[:-1] + np.maximum(length[:-1], 0)
    if bad.any():
        raise ValueError('row %d of the segment table is out of order or overlaps its predecessor' % int(np.flatnonzero(bad)[0]))
    return off, length


class CensusRun(object):
    """One census over a stream on the device: the table uploaded, the accumulator zeroed, a workspace for windows of up
    to ``window_bytes``.  ``add`` enqueues a window and waits for nothing; ``words`` synchronises once, raises on the
    status words and gives the ``n_seq x 16`` words back."""

    def __init__(self, torch, dev, seq_off, seq_len, window_bytes, min_gap=1):
        self.torch, self.dev, self.lib = torch, dev, _lib.load()
        self.n_seq, self.min_gap, self.window_bytes = int(len(seq_off)), int(min_gap), int(window_bytes)
        as_dev = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))
        self._off = as_dev(seq_off).to(device=dev, dtype=torch.int64).contiguous()
        self._len = as_dev(seq_len).to(device=dev, dtype=torch.int64).contiguous()       # (32 bits wide in the store)
        self._acc = torch.zeros((max(self.n_seq, 1), WORDS), dtype=torch.int64, device=dev)
        self._status = torch.full((2,), -1, dtype=torch.int64, device=dev)
        ws = self.lib.besst_dev_seq_census_workspace_bytes(self.window_bytes, self.n_seq)
        if not ws:
            raise BesstDeviceError('besst_dev_seq_census_workspace_bytes: a window of %d bytes is out of range' % self.window_bytes)
        self._ws = torch.empty(ws, dtype=torch.uint8, device=dev)

    def add(self, ptr, origin, n, stream=None):
        """Bytes [origin, origin + n) of the stream lie at device address ``ptr``."""
        if n > self.window_bytes:
            raise ValueError('a window of %d bytes on a workspace for %d' % (n, self.window_bytes))
        if stream is None:
            stream = self.torch.cuda.current_stream(self.dev)
        p = _C.c_void_p
        _lib.check(self.lib.besst_dev_seq_census(
            p(stream.cuda_stream), p(ptr), int(origin), int(n), self.n_seq, p(self._off.data_ptr()), p(self._len.data_ptr()),
            self.min_gap, p(self._ws.data_ptr()), p(self._acc.data_ptr()), p(self._status.data_ptr())), 'besst_dev_seq_census')

    def words(self):
        self.torch.cuda.synchronize(self.dev)
        status = self._status.cpu().numpy()
        if int(status[0]) != -1:
            raise BesstDeviceError('besst_dev_seq_census: row %d of the segment table is out of order or overlaps its '
                                   'predecessor' % int(status[0]))
        return self._acc[:self.n_seq].cpu().numpy()

    def close(self):
        self._off = self._len = self._acc = self._status = self._ws = None


def census_store(store, rows=None, min_gap=1):
    """The census of the store's contigs, in one call over the pool -> SequenceCensus (partial; ``finalised()`` closes
    the ends) of ``rows`` (default: every row, in order), named by the store."""
    from . import GenerateOutput as GO
    torch, dev = GO._torch_device(store.device.index)
    n = len(store)
    if rows is None:
        rows = np.arange(n, dtype=np.int64)
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    if len(rows) and (int(rows.min()) < 0 or int(rows.max()) >= n):
        raise ValueError('a row outside the sequence store')
    check_table(store.offsets, store.lengths)
    with torch.cuda.device(dev):
        run = CensusRun(torch, dev, store._off, store._len, store.pool_bytes, min_gap)
        try:
            if n and store.pool_bytes:
                run.add(store.pool_ptr, 0, store.pool_bytes)
            words = run.words()
        finally:
            run.close()
    return SequenceCensus([store.name_of(r) for r in rows.tolist()], words[rows], min_gap)


def census_source(src, seq_off, seq_len, window_bytes=None, min_gap=1):
    """The census of the segments [seq_off, seq_off + seq_len) (ascending, disjoint) of the file a ``ByteSource`` produces
    -> the ``n_seq x 16`` partial words.  The file is emitted window by window (``window_bytes``, GenerateOutput.CHUNK_BYTES
    by default) into one scratch buffer and counted there; ``src.check()`` runs at the end and raises what the source
    found wrong."""
    from . import GenerateOutput as GO
    torch, dev = src.torch, src.dev
    window = int(GO.CHUNK_BYTES if window_bytes is None else window_bytes)
    if window < 1:
        raise ValueError('window_bytes must be positive')
    seq_off, seq_len = check_table(seq_off, seq_len)
    total = int(src.total)
    window = max(1, min(window, total))
    with torch.cuda.device(dev):
        run = CensusRun(torch, dev, seq_off, seq_len, window, min_gap)
        try:
            buf = GO._out_buffer(torch, dev, window)
            stream = torch.cuda.current_stream(dev)
            for begin in range(0, total, window):
                end = min(begin + window, total)
                src.emit(begin, end, buf, stream)
                run.add(buf.data_ptr(), begin, end - begin, stream)
            src.check()
            return run.words()
        finally:
            run.close()


def write_stats(path, contigs, scaffolds):
    """assembly_stats.tsv: one row per metric, the input baseline (None: the column is left out) beside the scaffolds."""
    with open(path, 'w') as fh:
        print('\t'.join(['metric'] + (['contigs'] if contigs is not None else []) + ['scaffolds']), file=fh)
        before = dict(contigs.rows()) if contigs is not None else {}
        for metric, value in scaffolds.rows():
            print('\t'.join([metric] + ([_fmt(before[metric])] if contigs is not None else []) + [_fmt(value)]), file=fh)


def write_pass_report(em, Information, pass_dir, param):
    """PrintOutput's part of ``param.assembly_report``: pass<n>/scaffold_report.tsv and assembly_stats.tsv from the census
    of the scaffold FASTA as ``em`` emits it, and the before -> after lines in ``Information``.  Nothing changes the run."""
    census = em.report(min_gap=getattr(param, 'report_min_gap', 1)).finalised()
    census.write(pass_dir + '/scaffold_report.tsv')
    after, before = AssemblyStats(census), getattr(param, 'contig_stats', None)
    write_stats(pass_dir + '/assembly_stats.tsv', before, after)
    was = (lambda k: _fmt(getattr(before, k))) if before is not None else (lambda k: '-')
    print('Assembly report: N50 %s -> %s, L50 %s -> %s' % (was('N50'), _fmt(after.N50), was('L50'), _fmt(after.L50)),
          file=Information)
    print('Assembly report: sequences %s -> %s' % (was('n'), after.n), file=Information)
    print('Assembly report: total length %s -> %s' % (was('total'), after.total), file=Information)
    print('Assembly report: gaps %d (of at least %d N), gap bases %d' % (after.gaps, census.min_gap, after.gap_bases),
          file=Information)
    print('Assembly report: bases removed by overlap merges: %d' % int(np.asarray(em.layout.drop).sum()), file=Information)
    n60 = reference_n60(census.words[:, LEN])
    threshold = getattr(param, 'ins_size_threshold', None)
    if n60 is not None and threshold is not None and getattr(param, 'extend_paths', False) and n60 < threshold:
        print('Assembly report: note - N60 of these scaffolds (%d) is below the insert size threshold (%s): runBESST would '
              'switch to path finding here (decide_approach); this run goes on unchanged' % (n60, threshold), file=Information)
    return census, after
