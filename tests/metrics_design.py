"""Designed record streams for the library-metrics pass (csrc/metrics.hip) and the proof that each border case is in them.
Plain numpy; nothing here is imported from, or computed by, the kernels under test.

The pass keeps two ordered "first 1,000,000" lists - A (insert sizes) and D within B's cut-off (contamination).  A drawn
library meets their cut-offs wherever its seed puts them; the streams below are short, and a case is a stream plus the
running counts `before` = (a0, b0, d0) the scan starts from (pipeline.DeviceMetricsSampler.emit), chosen so that a cut-off
falls on one chosen record.  cases_present() then shows - from the MODEL's flag arrays (tests/dist_util.OracleMetricsBackend),
not from what the generator meant - that the cut lies on the record, lane, wave, sub-tile and tile the case's name says, and
mutant_kills() that each of a handful of subtly wrong models differs from the right one on at least one named case.

Every A or D record carries |tlen| = 1 + its index in the stream (never 0, and a misplaced value shows); the sign is what
its predicate needs.  Structural streams are scanned with min_mapq 10 and read_len 0.5, so that `read_len < |tlen|` holds
for every record; the two numeric comparisons have their own stream (value_stream)."""
import collections
import os
import re

import numpy as np
import torch

from tests.dist_util import OracleMetricsBackend
from besst_amd.records import RecordBatch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS_HIP = os.path.join(REPO, 'besst_amd', 'csrc', 'metrics.hip')

# ---- the kernel's geometry, each with the line of metrics.hip it mirrors ---------------------------------------------
LANES = 64                 # a wave of gfx950
THREADS = 256              # :22 kMetThreads
VEC = 4                    # :23 kMetVec: records per thread (and sub-tile)
SUB = THREADS * VEC        # :24 kMetTile: 1024 records per sub-tile
WAVE_RECORDS = LANES * VEC  # 256 records of a sub-tile per wave
SUBS = 4                   # :234 BESST_MET_SUBS
TILE = SUBS * SUB          # :237 kMetBig: 4096 records per tile
CAP = 1_000_000            # :25 kSampleCap
COUNT_TURN = 1024          # :190 blocks (of SUB records) per turn of the count-only scan
TILES_WAVES = 16           # :351 metrics_tiles_kernel: 1024 threads

MIN_MAPQ = 10
READ_LEN = 0.5


def tiles_per_wave(nt):
    """:359 per = roundup64(ceil(nt / 16)): the run of tiles a wave of metrics_tiles_kernel takes, in rounds of 64."""
    return (((nt + 15) // 16) + 63) & ~63


def source_constants():
    """The same constants as metrics.hip states them (for the CPU test)."""
    text = open(METRICS_HIP).read()

    def one(pattern):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))
    assert re.search(r'per = \(\(\(nt \+ 15u\) / 16u\) \+ 63u\) & ~63u', text)
    assert re.search(r'c0 < nblocks; c0 \+= 1024\)', text)
    return dict(THREADS=one(r'kMetThreads = (\d+);'), VEC=one(r'kMetVec = (\d+);'), SUBS=one(r'#define BESST_MET_SUBS (\d+)'),
                CAP=one(r'kSampleCap = (\d+);'))


def where(i):
    """(tile, sub-tile, wave, lane, record of the thread) of record i of a scan that starts at record 0."""
    w = i % TILE
    t = (w % SUB) // VEC
    return (i // TILE, w // SUB, t // LANES, t % LANES, i % VEC)


def where_str(i):
    return 't%d s%d w%d l%d r%d' % where(i)


# ---- records -----------------------------------------------------------------------------------------------------------
NON_TOP, K_A, K_D, K_PLAIN, K_UNMAPPED = range(5)
N_CONTIGS = 8
TOP_MASK = np.array([1, 0, 1, 1, 0, 0, 0, 1], np.uint8)        # top[0] = 1: what eval_tile:126's clamp reads for a bad id
TOP_IDS = np.array([0, 2, 3, 7], np.int32)
NON_TOP_IDS = np.array([-1, 1, 4, 5, 6, N_CONTIGS, N_CONTIGS + 1, 1 << 20, np.iinfo(np.int32).max, np.iinfo(np.int32).min],
                       np.int32)


def make_batch(kind, orientation):
    """Records of the given kinds.  A and D records alternate between the two forms of their predicate (read reverse /
    mate reverse); a record that is not on a top contig looks like an A record in every other respect."""
    n = len(kind)
    idx = np.arange(n, dtype=np.int64)
    val = (1 + idx).astype(np.int32)
    tid = np.where(kind == NON_TOP, NON_TOP_IDS[idx % len(NON_TOP_IDS)], TOP_IDS[idx % len(TOP_IDS)]).astype(np.int32)
    form = (idx // 3) % 2                                        # 0: mate reverse, 1: read reverse
    innie = (kind == K_D) if orientation == 'rf' else (kind != K_D)
    # innie: mate reverse and tlen > 0, or read reverse and tlen < 0; outie: the other sign (bam_parser.py:22-29)
    positive = (form == 0) == innie
    flag = np.where(form == 0, 0x80 | 0x1 | 0x20, 0x80 | 0x1 | 0x10).astype(np.uint16)
    plain = (kind == K_PLAIN) | (kind == K_UNMAPPED)
    flag[plain] = 0x40 | 0x1
    flag[kind == K_UNMAPPED] |= 0x4
    tlen = np.where(positive | plain, val, -val).astype(np.int32)
    z = np.zeros(n, np.int32)
    return RecordBatch(['c%d' % i for i in range(N_CONTIGS)], [1000] * N_CONTIGS, tid=tid, mtid=tid.copy(), pos=z, mpos=z,
                       tlen=tlen, flag=flag, mapq=np.full(n, 60, np.uint8), qlen=np.full(n, 100, np.uint16))


Case = collections.namedtuple('Case', 'name before want_isize claims consistent read_len min_mapq')


def _case(name, before, claims, want_isize=True, consistent=None, read_len=READ_LEN, min_mapq=MIN_MAPQ):
    a0, b0, d0 = before
    if consistent is None:
        consistent = True
        assert a0 + d0 <= b0, name                              # A and D are disjoint subsets of B
    return Case(name, tuple(int(x) for x in before), want_isize, claims, consistent, read_len, min_mapq)


class CachedModel(OracleMetricsBackend):
    """The model with its flag arrays kept per setting (a case only changes `before`); behaviour unchanged."""

    def __init__(self, batch, top):
        OracleMetricsBackend.__init__(self, batch, top)
        self._kept = {}

    def _flags(self, orientation, min_mapq, read_len):
        key = (orientation, min_mapq, read_len)
        if key not in self._kept:
            self._kept[key] = OracleMetricsBackend._flags(self, orientation, min_mapq, read_len)
        return self._kept[key]


class Stream(object):
    def __init__(self, name, kind, cases, cut_tiles=(), empty_tiles=(), batches=None):
        self.name = name
        self.kind = kind
        self.n = len(kind)
        self.cases = cases
        self.cut_tiles = tuple(cut_tiles)
        self.empty_tiles = tuple(empty_tiles)
        self.top = TOP_MASK
        self._batches = batches or {}
        self._models = {}
        names = [c.name for c in cases]
        assert len(set(names)) == len(names), 'case names repeat'

    def batch(self, orientation):
        if orientation not in self._batches:
            self._batches[orientation] = make_batch(self.kind, orientation)
        return self._batches[orientation]

    def model(self, orientation):
        if orientation not in self._models:
            self._models[orientation] = CachedModel(self.batch(orientation), self.top)
        return self._models[orientation]


# ---- dense stream --------------------------------------------------------------------------------------------------------
DENSE_N = 3 * TILE + 5                                          # 12293: three tiles and a ragged one of 5 records


DENSE_B_KS = [0, 1, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8192, DENSE_N - 1, DENSE_N, DENSE_N + 1]
DENSE_A_KS = [0, 1, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1365, 1366, 1367, 4095, 4096, 4097]   # (+ the A count, + 1, 8192)


def _dense_kind(n=DENSE_N):
    i = np.arange(n)
    kind = np.where(i % 3 == 0, K_A, np.where(i % 3 == 1, K_D, K_PLAIN)).astype(np.int8)
    # every other plain record is unmapped (C != B) - but not the last record inside a designed cut of B nor the first
    # behind it: an unmapped plain record adds to no count, and a cut wrong by that one record would not show
    ks = DENSE_B_KS + [k - 5 for k in DENSE_A_KS] + DENSE_A_KS
    near = np.isin(i, [k - 1 for k in ks] + ks)
    kind[((i % 6) == 5) & ~near] = K_UNMAPPED
    return kind


def dense_stream():
    n = DENSE_N
    kind = _dense_kind()
    n_a = int((kind == K_A).sum())
    cases = []
    # B's cut-off after k top records (every record is one): the last record inside is record k - 1
    for j, k in enumerate(DENSE_B_KS):
        d0 = 7 if j % 2 else 0
        if k == 0:
            claims, tag = dict(b='full', a='open'), 'full from the start'
        elif k > n:
            claims, tag = dict(b='open', a='open'), 'never reached'
        else:
            claims, tag = dict(b='cut', b_last=k - 1, a='open', named='B'), where_str(k - 1)
        cases.append(_case('B k=%d d0=%d: %s' % (k, d0, tag), (1000, CAP - k, d0), claims))
    # A's cap after k A records (every third record): the last one taken is record 3 (k - 1).  B either full from the start
    # (live_b false: D is not staged) or with as much room as a0 + d0 <= b0 leaves it, which puts its cut in front of A's.
    for k in DENSE_A_KS + [n_a, n_a + 1, 8192]:
        a_claim = dict(a='full') if k == 0 else dict(a='open') if k > n_a else dict(a='cut', a_last=3 * (k - 1), named='A')
        a_tag = 'full' if k == 0 else 'never reached' if k > n_a else where_str(3 * (k - 1))
        cases.append(_case('A k=%d, B full: %s' % (k, a_tag), (CAP - k, CAP + 3, 2), dict(a_claim, b='full')))
        d0 = 5 if k > 5 else 0
        kb = k - d0
        b_claim = dict(b='full') if kb == 0 else dict(b='cut', b_last=kb - 1)
        cases.append(_case('A k=%d, B k=%d d0=%d: %s' % (k, kb, d0, a_tag), (CAP - k, CAP - kb, d0), dict(a_claim, **b_claim)))
    # the relationships between the two cuts.  A real prefix has a0 <= b0 and A is a subset of B, so A never fills before
    # B: "A's cut in an earlier tile" can only be asked of the kernel with counts no stream produces (consistent=False:
    # held against the model, which treats the lists independently as the kernel does, but not against the C oracle).
    cases.append(_case('relation: A cut in tile 0, B cut in tile 1 (no real prefix)', (CAP - 10, CAP - 5000, 0),
                       dict(a='cut', a_last=27, b='cut', b_last=4999, relation='A earlier'), consistent=False))
    cases.append(_case('relation: both cuts in tile 0', (CAP - 100, CAP - 100, 0),
                       dict(a='cut', a_last=297, b='cut', b_last=99, relation='same tile')))
    cases.append(_case('relation: B cut in tile 0, A cut in tile 2', (CAP - 4000, CAP - 3000, 1000),
                       dict(a='cut', a_last=11997, b='cut', b_last=2999, relation='A later')))
    cases.append(_case('both full exactly, d0=0', (CAP, CAP, 0), dict(a='full', b='full')))
    cases.append(_case('both full exactly, d0=12 (no real prefix)', (CAP, CAP, 12), dict(a='full', b='full'), consistent=False))
    cases.append(_case('both full, past the cap', (CAP + 5, CAP + 77, 12), dict(a='full', b='full')))
    cases.append(_case('no insert sizes wanted, B cut in tile 1', (500, CAP - 4097, 3), dict(a='off', b='cut', b_last=4096),
                       want_isize=False))
    cases.append(_case('no insert sizes wanted, B full', (500, CAP, 3), dict(a='off', b='full'), want_isize=False))
    return Stream('dense', kind, cases)


# ---- sparse streams ------------------------------------------------------------------------------------------------------
# The top records of a cut tile, as (sub-tile, wave, lane, record): waves 1 and 3 only, so that waves 0 and 2 of the tile hold
# no top record (tile_flags returns false for them) and wave 0 lies in front of every cut.
CUT_PLACES = [(0, 1, 0, 0), (0, 1, 63, 3), (1, 3, 0, 2), (2, 1, 17, 1), (2, 3, 63, 0), (3, 1, 5, 3), (3, 3, 63, 3)]
CUT_KINDS = [K_D, K_A, K_UNMAPPED, K_D, K_PLAIN, K_A, K_D]
RAGGED_OFFS = [0, 2, 4]                                        # the ragged last tile holds five records
RAGGED_KINDS = [K_D, K_A, K_D]


def _offset(place):
    s, w, l, r = place
    return s * SUB + w * WAVE_RECORDS + l * VEC + r


def sparse_stream(name, n_tiles, cut_tiles, empty_tiles, seed, a_tiles=None):
    """n_tiles whole tiles and five records: 0..40 top records per tile at seeded places, none in empty_tiles, the designed
    ones in cut_tiles; a tile behind a cut tile holds at least eight (it begins at exactly 1,000,000 in one case)."""
    n = n_tiles * TILE + 5
    rng = np.random.default_rng(seed)
    kind = np.zeros(n, np.int8)
    tops = {}
    for t in range(n_tiles + 1):
        lo = t * TILE
        size = min(TILE, n - lo)
        if t in cut_tiles:
            offs = np.array([_offset(p) for p in CUT_PLACES] if size == TILE else RAGGED_OFFS)
            kinds = np.array(CUT_KINDS if size == TILE else RAGGED_KINDS)
        elif t in empty_tiles:
            continue
        else:
            c = int(rng.integers(0, 41))
            if t - 1 in cut_tiles:
                c = max(c, 8)
            c = min(c, size)
            offs = np.sort(rng.choice(size, c, replace=False))
            kinds = rng.choice([K_A, K_D, K_PLAIN, K_UNMAPPED], c, p=[0.35, 0.35, 0.15, 0.15])
            if t - 1 in cut_tiles and c:
                kinds[0], kinds[-1] = K_D, K_A
        kind[lo + offs] = kinds
        tops[t] = lo + offs
    is_b = kind != NON_TOP
    is_a = kind == K_A
    cum_b, cum_a = np.cumsum(is_b), np.cumsum(is_a)
    cases = []
    for t in cut_tiles:
        mine = tops[t]
        # (the middle one: the fourth, fifth or sixth of seven - the third is unmapped, and a cut wrong by it would not show)
        picks = [('first', mine[0]), ('middle', mine[3 + t % 3 if len(mine) > 3 else 1]), ('last', mine[-1])]
        for rank, i in picks:
            i = int(i)
            cases.append(_case('B cut after the %s top record of tile %d: %s' % (rank, t, where_str(i)),
                               (123, CAP - int(cum_b[i]), 45), dict(b='cut', b_last=i, b_rank=rank, b_tile=t, a='open', named='B')))
        if a_tiles is not None and t not in a_tiles:
            continue
        a_mine = [int(i) for i in mine if kind[i] == K_A]
        for j, i in enumerate((a_mine[0], a_mine[-1])):
            a0 = CAP - int(cum_a[i])
            if j == 0:
                cases.append(_case('A cut in tile %d, B full: %s' % (t, where_str(i)), (a0, CAP + 1, 0),
                                   dict(a='cut', a_last=i, a_tile=t, b='full', named='A')))
            else:
                d0 = min(9, int(cum_a[i]) - 1)                   # (b0 = a0 + d0 stays below the cap)
                cases.append(_case('A cut in tile %d, B cut in front of it: %s' % (t, where_str(i)), (a0, a0 + d0, d0),
                                   dict(a='cut', a_last=i, a_tile=t, b='cut', named='A')))
    return Stream(name, kind, cases, cut_tiles, empty_tiles)


SMALL_TILES = 65


def small_sparse_stream():
    # 66 tiles: `per` = 64, wave 0 of the tiles kernel takes tiles 0..63, wave 1 tiles 64 and 65
    return sparse_stream('sparse-small', SMALL_TILES, (0, 63, 64, 65), (5, 31, 62), 20251)


LARGE_TILES = 1024


def large_sparse_stream():
    # 1025 tiles: `per` = 128, two rounds of 64 per wave; tile 1024 is the ragged one
    return sparse_stream('sparse-large', LARGE_TILES, (0, 63, 64, 127, 128, 1023, 1024), (62, 126, 500, 1022), 20252, a_tiles=(127, 1024))


def count_stream():
    """1,048,576 + 1025 records for the count-only form: 1026 blocks of 1024, a second turn of its scan (:190)."""
    s = sparse_stream('sparse-count', 257, (), (3,), 20253)
    n = COUNT_TURN * SUB + 1025
    return Stream('sparse-count', s.kind[:n].copy(), [])


# ---- value borders -------------------------------------------------------------------------------------------------------
VALUE_READ_LENS = (100.0, 100.38)
VALUE_MIN_MAPQS = (0, 10, 254)


def value_stream():
    """`read_len < |tlen|` at equality (|tlen| 99, 100, 101 against read_len 100.0 and 100.38) and `mapq > min_mapq` at
    min_mapq, min_mapq + 1 and 255 for min_mapq 0, 10, 254: every combination with both signs of tlen, both forms of the
    orientation bits and read 1 / read 2.  The same records serve both orientations (what is an innie for one is the
    other's opposite pair)."""
    rows = [(at, sign, form, mapq, read2) for read2 in (1, 0) for at in (99, 100, 101) for sign in (1, -1) for form in (0, 1)
            for mapq in (0, 1, 10, 11, 254, 255)]
    n = len(rows)
    at, sign, form, mapq, read2 = [np.array(c) for c in zip(*rows)]
    flag = (np.where(read2 == 1, 0x80, 0x40) | 0x1 | np.where(form == 0, 0x20, 0x10)).astype(np.uint16)
    tid = TOP_IDS[np.arange(n) % len(TOP_IDS)]
    z = np.zeros(n, np.int32)
    batch = RecordBatch(['c%d' % i for i in range(N_CONTIGS)], [1000] * N_CONTIGS, tid=tid, mtid=tid.copy(), pos=z, mpos=z,
                        tlen=(at * sign).astype(np.int32), flag=flag, mapq=mapq.astype(np.uint8), qlen=np.full(n, 100, np.uint16))
    cases = [_case('read_len %r, min_mapq %d' % (rl, mq), (0, 0, 0), dict(), read_len=rl, min_mapq=mq)
             for rl in VALUE_READ_LENS for mq in VALUE_MIN_MAPQS]
    return Stream('values', np.full(n, K_PLAIN, np.int8), cases, batches={'fr': batch, 'rf': batch})


def value_cases_present(stream, orientation):
    b = stream.batch(orientation)
    m = stream.model(orientation)
    at = np.abs(b.tlen.astype(np.int64))
    read2 = (b.flag & 0x80) != 0
    for case in stream.cases:
        a, top, c, d = m._flags(orientation, case.min_mapq, case.read_len)
        assert top.all() and c.all()
        paired = a | d                                          # with every id a top one, the pairs that pass `base`
        mq = case.min_mapq
        # mapq: nothing at or below min_mapq, something at min_mapq + 1 and at 255
        assert not paired[b.mapq <= mq].any() and (b.mapq == mq).any(), case.name
        assert paired[b.mapq == min(mq + 1, 255)].any() and paired[b.mapq == 255].any(), case.name
        assert not paired[~read2].any()
        if orientation == 'rf':
            # D = innie and read_len < |tlen|: 100.0 < 100 fails, 100.0 < 101 holds; 100.38 < 100 fails, < 101 holds
            assert not d[at == 99].any() and not d[at == 100].any() and d[at == 101].any(), case.name
            assert a[at == 99].any() and a[at == 100].any()
        else:
            # D = outie and read_len < |tlen| + 2 read_len: holds for every length
            assert d[at == 99].any() and d[at == 100].any() and d[at == 101].any(), case.name
    return [c.name for c in stream.cases]


# ---- the model on flag arrays, and its mutants -----------------------------------------------------------------------------
MUTANTS = ('b_cap_plus_one', 'b_cap_minus_one', 'a_cap_plus_one', 'a_cap_minus_one', 'd_by_own_rank', 'c_past_the_cut',
           'inside_tile_left_to_the_straddle_path', 'tile_one_past_the_cap_taken_whole')


def mutants():
    """The wrong models cases_present / mutant_kills hold the cases against:
      b_cap_plus_one / minus_one   `rb < kSampleCap` (:467) off by one in either direction
      a_cap_plus_one / minus_one   the `room` clamp (:435) off by one in either direction
      d_by_own_rank                a D record admitted while D's own rank is below the cap, not B's
      c_past_the_cut               C counted for every top record, past B's cut
      inside_tile_left_to_the_straddle_path   `<=` read as `<` at :402 only: the tile that ends at exactly 1,000,000 is not
                                   counted as wholly inside, and nobody re-evaluates it (:439 still takes it as inside)
      tile_one_past_the_cap_taken_whole       the reverse: a tile whose last top record is the 1,000,001st is taken as
                                   wholly inside (`<=` against kSampleCap + 1 at :402 and :439)"""
    return MUTANTS


class Flags(object):
    def __init__(self, a, b, c, d, at):
        self.a, self.b, self.c, self.d, self.at = a, b, c, d, at
        self.n = len(a)
        self.cum_a, self.cum_b, self.cum_d = np.cumsum(a), np.cumsum(b), np.cumsum(d)
        starts = np.arange(0, max(self.n, 1), TILE)
        self.tile_of = np.arange(self.n) // TILE
        self.nb_t = np.add.reduceat(b.astype(np.int64), starts) if self.n else np.zeros(0, np.int64)
        self.pb_rel = np.cumsum(self.nb_t) - self.nb_t           # B records in front of each tile, within the stream
        # the top records alone (every flag is a subset of b): what emit_lists works on
        ix = np.nonzero(b)[0]
        self.t_a, self.t_c, self.t_d, self.t_at, self.t_tile = a[ix], c[ix], d[ix], at[ix], ix // TILE
        self.t_cum_a, self.t_cum_d, self.t_cum_b = self.cum_a[ix], self.cum_d[ix], self.cum_b[ix]


def flags_of(stream, orientation, case=None):
    m = stream.model(orientation)
    rl, mq = (case.read_len, case.min_mapq) if case is not None else (READ_LEN, MIN_MAPQ)
    a, b, c, d = m._flags(orientation, mq, rl)
    return Flags(a, b, c, d, m.at)


def emit_lists(F, before, want_isize, mutant=None):
    """-> (isize positions, values, contamination positions, values, counter_total, n_contam) of a scan of F's records
    that continues from `before`; mutant: one of mutants()."""
    a0, b0, d0 = before
    cap_a = CAP + (mutant == 'a_cap_plus_one') - (mutant == 'a_cap_minus_one')
    cap_b = CAP + (mutant == 'b_cap_plus_one') - (mutant == 'b_cap_minus_one')
    if want_isize:
        pos_a = a0 + F.t_cum_a - 1
        sel = F.t_a & (pos_a < cap_a)
        ia, va = pos_a[sel], F.t_at[sel]
    else:
        ia, va = np.zeros(0, np.int64), np.zeros(0, np.int64)
    inside = b0 + F.t_cum_b - 1 < cap_b
    pb_t = b0 + F.pb_rel
    if mutant == 'tile_one_past_the_cap_taken_whole':
        whole = (pb_t + F.nb_t == CAP + 1) & (F.nb_t > 0)
        inside = inside | whole[F.t_tile]
    pos_d = d0 + F.t_cum_d - 1
    sel_d = F.t_d & ((pos_d < CAP) if mutant == 'd_by_own_rank' else inside)
    n_c = int((F.t_c if mutant == 'c_past_the_cut' else F.t_c & inside).sum())
    n_d = int(sel_d.sum())
    if mutant == 'inside_tile_left_to_the_straddle_path':
        lost = (pb_t + F.nb_t == CAP) & (F.nb_t > 0)
        mine = lost[F.t_tile]
        n_c -= int((F.t_c & inside & mine).sum())
        n_d -= int((sel_d & mine).sum())
    return ia, va, pos_d[sel_d], F.t_at[sel_d], n_c, n_d


def _same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def buffer_of(lists):
    ia, va, idd, vd = lists[:4]
    out = np.zeros(2 * CAP, np.int32)
    out[ia] = va
    out[CAP + idd] = vd
    return out


# ---- the proof -----------------------------------------------------------------------------------------------------------
def _check_cut(name, flag, cum, before0, claim, last, what, named):
    """The list's state as the flags have it against the case's claim; -> the last record taken (None: no cut)."""
    rank = before0 + cum - 1
    total = before0 + (int(cum[-1]) if len(cum) else 0)
    if claim == 'full':
        assert before0 >= CAP, name
        return None
    if claim == 'open':
        assert total < CAP, name
        return None
    assert claim == 'cut' and before0 < CAP <= total, name
    hit = np.nonzero(flag & (rank == CAP - 1))[0]
    assert len(hit) == 1, name
    i = int(hit[0])
    if last is not None:
        assert i == last, '%s: %s fills on record %d (%s)' % (name, what, i, where_str(i))
        assert not named or where_str(i) in name, name
    return i


def cases_present(stream, orientation, agree_every=1):
    """Every case of the stream holds what its name and claims say, as the model's flags have it; the model here
    (emit_lists) and tests/dist_util.OracleMetricsBackend agree on every agree_every-th case.  -> {case name: facts found}."""
    if stream.name == 'values':
        return value_cases_present(stream, orientation)
    F = flags_of(stream, orientation)
    n, kind = stream.n, stream.kind
    nt = -(-n // TILE)
    per = tiles_per_wave(nt)
    # the stream itself
    assert np.array_equal(F.b, kind != NON_TOP) and np.array_equal(F.a, kind == K_A) and np.array_equal(F.d, kind == K_D)
    assert np.array_equal(F.c, F.b & (kind != K_UNMAPPED)) and (F.b & ~F.c).any()
    vals = F.at[F.a | F.d]
    assert np.array_equal(vals, 1 + np.nonzero(F.a | F.d)[0])
    if stream.name == 'dense':
        assert n == DENSE_N == 12293 and F.b.all() and n % VEC == 1
    else:
        tid = stream.batch(orientation).tid
        assert TOP_MASK[0] == 1 and (tid[~F.b] == -1).any() and (tid[~F.b] >= N_CONTIGS).any()
        assert (n - 5) % TILE == 0 and n % TILE == 5
        assert per == (64 if nt <= 1024 else 128)
        assert F.nb_t.max() <= 40 and F.nb_t.min() == 0
        for t in stream.empty_tiles:
            assert F.nb_t[t] == 0
        assert any(t + 1 in stream.cut_tiles for t in stream.empty_tiles)        # nothing just in front of a cut tile
        tops = np.nonzero(F.b)[0]
        assert len({where(i)[1] for i in tops}) == SUBS and len({where(i)[2] for i in tops}) == THREADS // LANES
        assert len({where(i)[3] for i in tops}) == LANES and len({where(i)[4] for i in tops}) == VEC
        # where the cut tiles sit in the tiles kernel: round and wave borders, the ragged last tile
        sits = {(t // per, (t % per) // 64, t % 64) for t in stream.cut_tiles}
        if nt <= 1024:
            assert {(0, 0, 0), (0, 0, 63), (1, 0, 0), (1, 0, 1)} <= sits and nt - 1 in stream.cut_tiles
        else:
            assert {(0, 0, 0), (0, 0, 63), (0, 1, 0), (0, 1, 63), (1, 0, 0), (7, 1, 63), (8, 0, 0)} <= sits
            assert nt - 1 == 1024 in stream.cut_tiles
    found = {}
    relations, b_ranks, a_kinds = set(), set(), set()
    model = stream.model(orientation)
    for number, case in enumerate(stream.cases):
        a0, b0, d0 = case.before
        cl = case.claims
        name = '%s / %s / %s' % (stream.name, orientation, case.name)
        if case.consistent:
            assert a0 + d0 <= b0, name
        bi = _check_cut(name, F.b, F.cum_b, b0, cl['b'], cl.get('b_last'), 'B', cl.get('named') == 'B')
        ai = None
        if cl['a'] == 'off':
            assert not case.want_isize, name
        else:
            assert case.want_isize, name
            ai = _check_cut(name, F.a, F.cum_a, a0, cl['a'], cl.get('a_last'), 'A', cl.get('named') == 'A')
        facts = dict(b_last=bi, a_last=ai)
        pb_t = b0 + F.pb_rel
        straddle = np.nonzero((pb_t < CAP) & (pb_t + F.nb_t > CAP))[0].tolist()
        if bi is None:
            assert straddle == [], name
        else:
            t = bi // TILE
            in_tile = np.nonzero(F.b[t * TILE:(t + 1) * TILE])[0] + t * TILE
            rank = 'last' if bi == in_tile[-1] else 'first' if bi == in_tile[0] else 'middle'
            if len(in_tile) == 1:
                rank = 'only'
            facts['b_rank'] = rank
            b_ranks.add(rank)
            if 'b_rank' in cl:
                assert rank == cl['b_rank'] and t == cl['b_tile'], name
            if rank in ('last', 'only'):
                # the `<=` border: the tile ends at exactly 1,000,000, no tile straddles, the next one with B > 0 begins there
                assert straddle == [] and pb_t[t] + F.nb_t[t] == CAP, name
                later = [u for u in range(t + 1, nt) if F.nb_t[u] > 0]
                if later:
                    assert pb_t[later[0]] == CAP, name
                    facts['next_begins_at_cap'] = later[0]
                    u = later[0]
                    assert F.d[u * TILE:(u + 1) * TILE].any() and F.c[u * TILE:(u + 1) * TILE].any(), name
            else:
                assert straddle == [t], name
                facts['straddle'] = t
                if 'b_rank' in cl and t != nt - 1:
                    # a wave of the straddling tile without a top record, in front of the cut's wave
                    wave_of = ((in_tile % SUB) // WAVE_RECORDS)
                    idle = set(range(THREADS // LANES)) - set(wave_of.tolist())
                    assert idle and min(idle) < where(bi)[2], name
                    facts['idle_wave_in_front'] = min(idle)
        if ai is not None and pb_t is not None:
            ta = ai // TILE
            if 'a_tile' in cl:
                assert ta == cl['a_tile'], name
            rel = 'B full' if cl['b'] == 'full' else None
            if bi is not None:
                rel = 'A earlier' if ta < bi // TILE else 'same tile' if ta == bi // TILE else 'A later'
            if 'relation' in cl:
                assert rel == cl['relation'], name
            facts['relation'] = rel
            relations.add(rel)
            a_kinds.add('ragged' if ta == nt - 1 else 'whole')
        # the two statements of the model agree
        lists = emit_lists(F, case.before, case.want_isize)
        if number % agree_every == 0:
            want, state = model.emit(torch.tensor(case.before), orientation, case.min_mapq, case.read_len, case.want_isize)
            assert np.array_equal(want.numpy(), buffer_of(lists)), name
            assert (int(state[3]), int(state[4]), int(state[5])) == (lists[4], lists[5], n), name
        # a cut wrong by one record in either direction shows on the very case that names the cut
        if cl.get('named') == 'B' and bi is not None and F.b[bi + 1:].any():
            for m in ('b_cap_plus_one', 'b_cap_minus_one', 'd_by_own_rank', 'c_past_the_cut'):
                assert not _same(lists, emit_lists(F, case.before, case.want_isize, m)), '%s: blind to %s' % (name, m)
        if cl.get('named') == 'A' and ai is not None and F.a[ai + 1:].any():
            for m in ('a_cap_plus_one', 'a_cap_minus_one'):
                assert not _same(lists, emit_lists(F, case.before, case.want_isize, m)), '%s: blind to %s' % (name, m)
        if cl['a'] in ('full', 'off'):
            assert len(lists[0]) == 0, name
        if cl['b'] == 'full':
            assert len(lists[2]) == 0 and lists[4] == 0, name
        found[case.name] = facts
    if stream.name == 'dense':
        assert relations >= {'A earlier', 'same tile', 'A later', 'B full'}
        assert b_ranks >= {'first', 'middle', 'last'}
        cut_at = {f['b_last'] for f in found.values() if f['b_last'] is not None}
        assert {0, 3, 4, 254, 255, 256, 1022, 1023, 1024, 4094, 4095, 4096, 8191, n - 2, n - 1} <= cut_at
        assert a_kinds == {'whole', 'ragged'}
    else:
        assert 'B full' in relations and relations & {'same tile', 'A later'}
        got = {(f['b_last'] // TILE, f['b_rank']) for f in found.values() if f.get('b_rank')}
        for t in stream.cut_tiles:
            assert {(t, 'first'), (t, 'middle'), (t, 'last')} <= got, t
    return found


def mutant_kills(streams, orientation):
    """{mutant: [names of the cases on which it differs from the right model]}; asserts that no list is empty."""
    kills = {m: [] for m in mutants()}
    for stream in streams:
        F = flags_of(stream, orientation)
        for case in stream.cases:
            right = emit_lists(F, case.before, case.want_isize)
            for m in mutants():
                if not _same(right, emit_lists(F, case.before, case.want_isize, m)):
                    kills[m].append('%s: %s' % (stream.name, case.name))
    for m, names in kills.items():
        assert names, 'no designed case tells the mutant %s from the right model' % m
    return kills


# ---- the host chunk loop ---------------------------------------------------------------------------------------------------
CHUNK = 16 << 20                                                # api.hip:1197 kChunk: the first chunk of besst_ctx_metrics_sample
CHUNK_TAIL = 1_300_000


def chunk_loop_stream(seed=20254):
    """A first chunk with 300 top records at seeded places - so that the second chunk is sized from a tiny rate - and a dense
    tail in which five records of six are A: B is cut in the second chunk, and A fills exactly, on a later record."""
    n = CHUNK + CHUNK_TAIL
    rng = np.random.default_rng(seed)
    kind = np.zeros(n, np.int8)
    at = np.sort(rng.choice(CHUNK, 300, replace=False))
    kind[at] = rng.choice([K_A, K_D, K_PLAIN, K_UNMAPPED], 300, p=[0.35, 0.35, 0.15, 0.15])
    j = np.arange(CHUNK_TAIL)
    kind[CHUNK:] = np.where(j % 6 < 5, K_A, np.where((j // 6) % 2 == 0, K_D, K_UNMAPPED))
    return Stream('chunk-loop', kind, [])


def chunk_loop_present(stream):
    """-> (record on which B is cut, record on which A fills): both in the second chunk, in this order."""
    kind = stream.kind
    assert stream.n == CHUNK + CHUNK_TAIL
    head_b = int((kind[:CHUNK] != NON_TOP).sum())
    assert 200 <= head_b <= 300 and (kind[CHUNK:] != NON_TOP).all()
    b_cut = int(np.searchsorted(np.cumsum(kind != NON_TOP), CAP))
    a_cut = int(np.searchsorted(np.cumsum(kind == K_A), CAP))
    assert CHUNK < b_cut < a_cut < stream.n - 1
    return b_cut, a_cut
