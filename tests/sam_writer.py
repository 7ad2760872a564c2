"""Test scaffolding: a RecordBatch as SAM text (bytes).  It shares no code with the product.

A record's CIGAR is ``[clip S] qlen M`` with clip = rlen - qlen, as besst_bam_write_records writes it (a record with
rlen = qlen = 0 gets '*'), so that the BAM and the SAM of one batch hold the same records.  SEQ is rlen bases ('*' for
rlen 0, or for every record with ``seq_star`` - then the CIGAR alone gives the lengths), QUAL as long as SEQ.
"""
import numpy as np


def qname(i, length=None):
    """'r<i>' padded with 'x' to ``length`` bytes (never cut below the number)"""
    name = 'r%d' % i
    return name if length is None else name + 'x' * max(0, length - len(name))


def header_text(references, lengths, hd=True):
    head = '@HD\tVN:1.4\tSO:unknown\n' if hd else ''
    return head + ''.join('@SQ\tSN:%s\tLN:%d\n' % (n, int(l)) for n, l in zip(references, lengths))


def record_line(i, references, tid, mtid, pos, mpos, tlen, flag, mapq, qlen, rlen, name_len=None, optional='', seq_star=False,
                rnext_equals=True):
    rname = '*' if tid < 0 else references[tid]
    if mtid < 0:
        rnext = '*'
    elif mtid == tid and rnext_equals:
        rnext = '='
    else:
        rnext = references[mtid]
    rlen = max(rlen, 0)
    clip = rlen - qlen
    cigar = ('%dS' % clip if clip > 0 else '') + ('%dM' % qlen if qlen > 0 else '') or '*'
    if seq_star or rlen == 0:
        seq = qual = '*'
    else:
        seq, qual = ('ACGT' * (rlen // 4 + 1))[:rlen], 'I' * rlen
    fields = [qname(i, name_len), str(flag), rname, str(pos + 1), str(mapq), cigar, rnext, str(mpos + 1), str(tlen), seq, qual]
    return '\t'.join(fields) + optional


def padded_references(batch):
    """The batch's references and lengths; a batch whose records name a reference id beyond its header (BAM stores any
    int32, SAM text can only name a header line) gets placeholder references 'unlisted_<id>' of length 1 behind them"""
    refs, lengths = list(batch.references), [int(x) for x in batch.lengths]
    top = max([len(refs) - 1] + [int(np.max(c)) for c in (batch.tid, batch.mtid) if len(c)])
    for k in range(len(refs), top + 1):
        refs.append('unlisted_%d' % k)
        lengths.append(1)
    return refs, lengths


def sam_bytes(batch, eol='\n', final_newline=True, name_len=None, optional='', seq_star=False, hd=True, order=None):
    """The batch as a SAM file.  name_len: an int or a function of the record's index; optional: text appended to every
    record line (begin it with a tab) or a function of the index; order: the record indices in file order."""
    rlen = batch.rlen if batch.rlen is not None else batch.qlen
    cols = [np.asarray(c).tolist() for c in (batch.tid, batch.mtid, batch.pos, batch.mpos, batch.tlen, batch.flag, batch.mapq,
                                             batch.qlen, rlen)]
    refs, lengths = padded_references(batch)
    lines = []
    for i in (range(len(cols[0])) if order is None else order):
        lines.append(record_line(i, refs, *[c[i] for c in cols],
                                 name_len=name_len(i) if callable(name_len) else name_len,
                                 optional=optional(i) if callable(optional) else optional, seq_star=seq_star))
    text = header_text(refs, lengths, hd).replace('\n', eol) + eol.join(lines)
    if lines and final_newline:
        text += eol
    return text.encode()
