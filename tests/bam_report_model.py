"""The BAM report restated in plain numpy from the eight record columns, and its digest in Python integers - what
besst_dev_library_report (csrc/report.hip) must equal word for word.  Shares no code with besst_amd/report.py: the rules and
the word layout are written out again here from the header's comment (include/besst_amd.h).
"""
import numpy as np

ROWS = ('in total', 'primary', 'secondary', 'supplementary', 'duplicates', 'primary duplicates', 'mapped', 'primary mapped',
        'paired in sequencing', 'read1', 'read2', 'properly paired', 'with itself and mate mapped', 'singletons',
        'with mate mapped to a different chr', 'with mate mapped to a different chr (mapQ>=5)')
COLUMNS = ('tid', 'mtid', 'pos', 'mpos', 'tlen', 'flag', 'mapq', 'qlen')
M64 = (1 << 64) - 1


def n_words(n_refs, isize_bins):
    return 40 + 256 + 65536 + 2 * n_refs + 3 * (isize_bins + 1)


def columns_of(batch):
    """{column: numpy array} of a RecordBatch (or of a dict that has them already)."""
    get = (lambda k: batch[k]) if isinstance(batch, dict) else (lambda k: getattr(batch, k))
    return {k: np.asarray(get(k)) for k in COLUMNS}


def splitmix64(x):
    x = (x + 0x9e3779b97f4a7c15) & M64
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & M64
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


def record_hash(tid, mtid, pos, mpos, tlen, flag, mapq, qlen):
    """One record's h, in Python integers."""
    u32 = lambda v: int(v) & 0xffffffff
    a = u32(tid) | u32(mtid) << 32
    b = u32(pos) | u32(mpos) << 32
    c = u32(tlen) | int(flag) << 32 | int(qlen) << 48
    return splitmix64(splitmix64(splitmix64(splitmix64(a) ^ b) ^ c) ^ int(mapq))


def digest_py(cols):
    """(sum mod 2^64, xor) of the records' h - the ten-line script over any decoder's records."""
    s = x = 0
    for rec in zip(*[cols[k].tolist() for k in COLUMNS]):
        h = record_hash(*rec)
        s = (s + h) & M64
        x ^= h
    return s, x


def _splitmix64_np(x):
    x = x + np.uint64(0x9e3779b97f4a7c15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def digest_np(cols):
    """digest_py in wrapping uint64 arithmetic (for the streams of millions of records; test_bam_report_model holds the two
    against each other)."""
    u = lambda k: cols[k].astype(np.int64).astype(np.uint64) & np.uint64(0xffffffff)
    with np.errstate(over='ignore'):
        a = u('tid') | u('mtid') << np.uint64(32)
        b = u('pos') | u('mpos') << np.uint64(32)
        c = u('tlen') | cols['flag'].astype(np.uint64) << np.uint64(32) | cols['qlen'].astype(np.uint64) << np.uint64(48)
        h = _splitmix64_np(_splitmix64_np(_splitmix64_np(_splitmix64_np(a) ^ b) ^ c) ^ cols['mapq'].astype(np.uint64))
        s = int(np.add.reduce(h, dtype=np.uint64)) if h.size else 0
        x = int(np.bitwise_xor.reduce(h)) if h.size else 0
    return s, x


def model(batch, n_refs, isize_bins=32768):
    """-> dict of the report's parts: census (16 x 2), unplaced, tid_out_of_range, pairs (4), digest, mapq, qlen, mapped,
    placed_unmapped, innie / outie / tandem (isize_bins + 1 each)."""
    c = columns_of(batch)
    tid, mtid = c['tid'].astype(np.int64), c['mtid'].astype(np.int64)
    tlen, f = c['tlen'].astype(np.int64), c['flag'].astype(np.int64)
    mapq, qlen = c['mapq'].astype(np.int64), c['qlen'].astype(np.int64)
    has = lambda bit: (f & bit) != 0
    fail, mapped = has(0x200), ~has(0x4)
    secondary = has(0x100)
    supplementary = ~secondary & has(0x800)
    primary = ~secondary & ~has(0x800)
    paired = primary & has(0x1)
    both = paired & mapped & ~has(0x8)
    diff = both & (tid != mtid)
    rows = [np.ones(f.shape, bool), primary, secondary, supplementary, has(0x400), primary & has(0x400), mapped,
            primary & mapped, paired, paired & has(0x40), paired & has(0x80), paired & has(0x2) & mapped, both,
            paired & has(0x8) & mapped, diff, diff & (mapq >= 5)]
    census = np.array([[int((r & ~fail).sum()), int((r & fail).sum())] for r in rows], dtype=np.int64)
    in_range = (tid >= 0) & (tid < n_refs)
    out = dict(census=census, unplaced=int((tid < 0).sum()), tid_out_of_range=int((tid >= n_refs).sum()))
    out['mapped'] = np.bincount(tid[in_range & mapped], minlength=n_refs).astype(np.int64)
    out['placed_unmapped'] = np.bincount(tid[in_range & ~mapped], minlength=n_refs).astype(np.int64)
    out['mapq'] = np.bincount(mapq[mapped], minlength=256).astype(np.int64)
    out['qlen'] = np.bincount(qlen[mapped], minlength=65536).astype(np.int64)
    geo = both & has(0x80) & (tid == mtid) & in_range
    rev, mrev = has(0x10), has(0x20)
    tandem = geo & (rev == mrev)
    opposite = geo & (rev != mrev)
    other = opposite & (tlen == 0)
    innie = opposite & ((rev & (tlen < 0)) | (~rev & (tlen > 0)))
    outie = opposite & ((rev & (tlen > 0)) | (~rev & (tlen < 0)))
    out['pairs'] = np.array([innie.sum(), outie.sum(), tandem.sum(), other.sum()], dtype=np.int64)
    size = np.minimum(np.abs(tlen), isize_bins)                   # (int64: |INT32_MIN| is 2^31)
    for name, sel in (('innie', innie), ('outie', outie), ('tandem', tandem)):
        out[name] = np.bincount(size[sel], minlength=isize_bins + 1).astype(np.int64)
    out['digest'] = digest_np(c) if f.shape[0] > 5000 else digest_py(c)
    return out


def words(batch, n_refs, isize_bins=32768):
    """The model as the report's 64-bit words (uint64), in the layout of include/besst_amd.h."""
    m = model(batch, n_refs, isize_bins)
    w = np.zeros(n_words(n_refs, isize_bins), dtype=np.uint64)
    w[0:32] = m['census'].reshape(-1).astype(np.uint64)
    w[32], w[33] = m['unplaced'], m['tid_out_of_range']
    w[34:38] = m['pairs'].astype(np.uint64)
    w[38], w[39] = np.uint64(m['digest'][0]), np.uint64(m['digest'][1])
    w[40:296] = m['mapq'].astype(np.uint64)
    w[296:65832] = m['qlen'].astype(np.uint64)
    at = 65832
    for key in ('mapped', 'placed_unmapped', 'innie', 'outie', 'tandem'):
        w[at:at + m[key].shape[0]] = m[key].astype(np.uint64)
        at += m[key].shape[0]
    assert at == w.shape[0]
    return w


def flag_table(n_refs=3, shuffled=None):
    """All 4096 values of flag & 0xfff crossed with tid == mtid / differ / tid = -1 / mtid = -1 -> columns of 16384 records in
    product order (``shuffled``: a seed, the same records in another order).  tlen, mapq and qlen vary with the index so that
    every class, both sides of mapQ 5 and several bins are met."""
    k = np.arange(4 * 4096)
    flag = (k % 4096).astype(np.uint16)
    case = k // 4096
    tid = np.where(case == 2, -1, k % n_refs).astype(np.int32)
    mtid = np.where(case == 0, tid, np.where(case == 3, -1, (tid + 1) % n_refs)).astype(np.int32)
    if n_refs == 1:
        mtid = np.where(case == 1, 7, mtid).astype(np.int32)          # (one reference: "differ" is a mate outside the header)
    cols = dict(tid=tid, mtid=mtid, pos=(k * 7 % 1000).astype(np.int32), mpos=(k * 11 % 1000).astype(np.int32),
                tlen=((k % 5 - 2) * (k % 701)).astype(np.int32), flag=flag, mapq=(k % 9).astype(np.uint8),
                qlen=(90 + k % 3).astype(np.uint16))
    if shuffled is not None:
        order = np.random.RandomState(shuffled).permutation(k.shape[0])
        cols = {key: np.ascontiguousarray(v[order]) for key, v in cols.items()}
    return cols
