"""Designed record streams for the record loop (csrc/classify.hip: stream_kernel + ordered_kernel, fused_wave_kernel<kRuns,
kBits>, the stitch and compact kernels) and a census of the structural borders each of them meets.  Plain numpy / Python;
nothing here is imported from, or computed by, the kernels under test.

A drawn library meets the kernels' borders - the 320-slot ring one short of full, a chunk closed by its run count, 64
against 65 chunks in a block, a block head that duplicates the block before - by accident or never.  The streams below place
them on purpose: `place` solves PosDirCalculatorPE/MP for the coordinate that gives a wanted observation, `replay` restates
the loop body (CreateGraph.py:111-211, 812-871) sequentially - with named WRONG variants of its rules, so that the CPU test
can show that each designed stream tells the right rule from the wrong one -, and `census` says, from the rules as the
source comments state them, where every designed record falls: sub-tile, queue depth, evaluation round, chunk, group.
tests/test_record_design.py checks all of that without a GPU; tests/test_gpu_record_borders.py sends every stream through
every form of the record loop."""
import collections
import functools
import math
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'besst_amd', 'csrc')

F_UNMAPPED, F_MUNMAPPED, F_REVERSE, F_MREVERSE, F_READ1, F_READ2 = 0x4, 0x8, 0x10, 0x20, 0x40, 0x80
CLS_ABSENT, CLS_LARGE, CLS_SMALL = 0, 1, 2
MASK_G, MASK_GP = 1, 2


# ---- the structural constants, read from the sources -------------------------------------------------------------------
def _knob(source, pattern):
    """The integer a source line gives a constant: `pattern` holds one group, a number or a product of numbers."""
    text = open(os.path.join(CSRC, source)).read()
    m = re.search(pattern, text)
    assert m, '%s: nothing matches %s' % (source, pattern)
    value = 1
    for part in m.group(1).split('*'):
        value *= int(part.strip().rstrip('u'))
    return value


def source_constants():
    c = {}
    c['kGroup'] = 64 * _knob('common.h', r'constexpr int kStreamVec = (\d+);')
    assert re.search(r'constexpr int kGroup = 64 \* kStreamVec;', open(os.path.join(CSRC, 'common.h')).read())
    c['kClsTile'] = _knob('common.h', r'#define\s+BESST_CAND_GROUPS\s+(\d+)') * c['kGroup']
    assert re.search(r'constexpr int kClsTile = kCandGroups \* kGroup;', open(os.path.join(CSRC, 'common.h')).read())
    c['kStreamTile'] = (_knob('common.h', r'constexpr int kStreamThreads = (\d+);') * _knob('common.h', r'constexpr int kStreamVec = (\d+);')
                        * _knob('common.h', r'#define\s+BESST_STREAM_SUBTILES\s+(\d+)'))
    c['kFwSub'] = _knob('classify.hip', r'constexpr int kFwSub = (\d+);')
    assert re.search(r'constexpr int kFwRing = kFwSub \+ 64;', open(os.path.join(CSRC, 'classify.hip')).read())
    c['kFwRing'] = c['kFwSub'] + 64
    assert re.search(r'constexpr int kOrdRound = kOrdWaves \* kAhead \* 64;', open(os.path.join(CSRC, 'classify.hip')).read())
    c['kOrdRound'] = (_knob('classify.hip', r'constexpr int kOrdWaves = (\d+);') * _knob('classify.hip', r'#define\s+BESST_ORD_AHEAD\s+(\d+)')
                      * 64)
    for name in ('kRlChunkTuples', 'kRlCloseRuns', 'kRlSlots', 'kRlMaxChunks'):
        c[name] = _knob('common.h', r'constexpr int %s = (\d+);' % name)
    assert re.search(r'constexpr uint32_t kStitchSpan = 1024u \* kStitchRounds;', open(os.path.join(CSRC, 'classify.hip')).read())
    c['kStitchSpan'] = 1024 * _knob('classify.hip', r'constexpr int kStitchRounds = (\d+);')
    return c


K = source_constants()
BLOCK, SUB, RING, GROUP = K['kClsTile'], K['kFwSub'], K['kFwRing'], K['kGroup']


# ---- the contig table ----------------------------------------------------------------------------------------------------
N_CONTIGS = 2560
LARGE_LEN, SMALL_LEN = 6000, 400
PAIR_GAP = 100


def make_table():
    """Rows in groups of eight: three large contigs on scaffolds of their own (forward, forward, reverse), one small forward,
    one small reverse, one absent, and the two contigs of ONE scaffold (the first forward at position 0, the second reverse
    behind a gap; every fourth such scaffold is of the small class).  Scaffold ids run to 2560: node codes of 13 bits, keys of
    27 - stage 2's hand-over from the record loop is on."""
    cls, scaf, slen, cpos, clen, cdir = [], [], [], [], [], []
    for r in range(N_CONTIGS):
        k, g = r % 8, r // 8
        if k in (0, 1, 2):
            row = (CLS_LARGE, r + 1, LARGE_LEN + g, 0, LARGE_LEN + g, k != 2)
        elif k in (3, 4):
            row = (CLS_SMALL, r + 1, SMALL_LEN + g % 50, 0, SMALL_LEN + g % 50, k == 3)
        elif k == 5:
            row = (CLS_ABSENT, 0, 0, 0, 0, True)
        else:
            small = g % 4 == 3
            a, b = (150, 120) if small else (3000, 2500)
            total = a + PAIR_GAP + b
            row = ((CLS_SMALL if small else CLS_LARGE), r - (k - 6) + 1, total, 0 if k == 6 else a + PAIR_GAP, a if k == 6 else b, k == 6)
        for col, v in zip((cls, scaf, slen, cpos, clen, cdir), row):
            col.append(v)
    return dict(cls=cls, scaf=scaf, slen=slen, cpos=cpos, clen=clen, cdir=cdir)


TABLE = make_table()
NODE_BITS = max(1, (max(TABLE['scaf']) * 2 + 1).bit_length())
assert max(TABLE['scaf']) >= 2048 and 2 * NODE_BITS + 1 >= 25


@functools.lru_cache(maxsize=None)
def rows_of(kind, forward=None):
    """Table rows of a kind: 'large', 'small' (scaffolds of one contig), 'absent', 'pair0' / 'pair1' (the two contigs of a
    large scaffold), 'spair0' / 'spair1' (of a small one)."""
    out = []
    for r in range(N_CONTIGS):
        k, g = r % 8, r // 8
        kd = ('large', 'large', 'large', 'small', 'small', 'absent', 'pair0', 'pair1')[k]
        if k >= 6 and g % 4 == 3:
            kd = 's' + kd
        if kd == kind and (forward is None or TABLE['cdir'][r] == forward):
            out.append(r)
    return tuple(out)


def table_columns(table=TABLE):
    """The table as the numpy columns the device entry points and the C oracle take."""
    return dict(scaf_id=np.asarray(table['scaf'], np.int32), scaf_len=np.asarray(table['slen'], np.int32),
                ctg_pos=np.asarray(table['cpos'], np.int32), ctg_len=np.asarray(table['clen'], np.int32),
                direction=np.asarray(table['cdir'], np.uint8), cls=np.asarray(table['cls'], np.uint8))


def make_lib(orientation='fr', read_len=100, threshold=800.0, min_mapq=11, detect_duplicate=True, extend_paths=True,
             no_score=False):
    return dict(orientation=orientation, read_len=read_len, ins_size_threshold=threshold, min_mapq=min_mapq,
                detect_duplicate=detect_duplicate, extend_paths=extend_paths, no_score=no_score)


# ---- PosDirCalculatorPE / MP (CreateGraph.py:1024-1076) and its inverse -----------------------------------------------------
def posdir(orientation, cdir, rdir, cpos, rpos, slen, clen, read_len):
    """One end -> (observation, side); side 1 = 'R'."""
    if orientation != 'fr':
        rdir = not rdir
    if cdir and rdir:
        return int(slen - cpos - rpos), 1
    if not cdir and rdir:
        return int(cpos + (clen - rpos)), 0
    if cdir:
        return int(cpos + rpos + read_len), 0
    return int(slen - cpos - (clen - rpos - read_len)), 1


def branch_of(lib, row, reverse, table=TABLE):
    """Which of the calculator's four branches a read with strand bit `reverse` takes on contig `row`: 0 .. 3 in the order of
    the reference's if-chain (the last two add read_len: the float branches of a fractional read length)."""
    rdir = not reverse
    if lib['orientation'] != 'fr':
        rdir = not rdir
    cdir = bool(table['cdir'][row])
    return {(True, True): 0, (False, True): 1, (True, False): 2, (False, False): 3}[(cdir, rdir)]


def place(row, reverse, obs, lib, table=TABLE):
    """The read position on contig `row` at which a read with strand bit `reverse` observes `obs` under `lib`."""
    cdir, cpos, slen, clen = bool(table['cdir'][row]), table['cpos'][row], table['slen'][row], table['clen'][row]
    rl = lib['read_len']
    b = branch_of(lib, row, reverse, table)
    guess = (slen - cpos - obs, cpos + clen - obs, math.floor(obs - cpos - rl), math.floor(obs - slen + cpos + clen - rl))[b]
    for pos in (guess, guess + 1, guess - 1, guess + 2):
        if posdir(lib['orientation'], cdir, not reverse, cpos, pos, slen, clen, rl)[0] == obs:
            return int(pos)
    raise AssertionError('no position gives observation %d on row %d' % (obs, row))


# ---- the loop body, restated (CreateGraph.py:111-211, 812-871) --------------------------------------------------------------
MUTATIONS = ('prev_from_kept', 'dup_on_o1_only', 'le_threshold', 'ge_25', 'floor_threshold', 'second_call_keeps_prev',
             'duplicate_still_calls_twice', 'coverage_with_absent_mate', 'mapq0_without_coverage', 'non_unique_read2_only')

Replay = collections.namedtuple('Replay', 'reach accept emit dup fishy key o1 o2 counters aligned prev n_reach tuples')


def replay(rec, table, lib, mutate=None):
    """-> Replay: per record reach / accept / emit (a link tuple) / dup (its first CreateEdge call met its own observations) /
    fishy (a BWA-quirk tuple), key ((n_min << node_bits | n_max) << 1 | fishy, -1 where the record has no node pair) and its
    observations; counters = [count, non_unique, non_unique_for_scaf, nr_of_duplicates, too_long, fishy_reads, n_tuples,
    n_reach, prev1, prev2]; the coverage numerators; the tuples (n_min, n_max, fishy, obs of n_min, obs of n_max, mask) in
    stream order.  mutate: one of MUTATIONS - the same loop with that rule wrong."""
    assert mutate is None or mutate in MUTATIONS, mutate
    cls, scaf, slen, cpos, clen, cdir = (table[k] for k in ('cls', 'scaf', 'slen', 'cpos', 'clen', 'cdir'))
    nc = len(cls)
    n = len(rec['tid'])
    fr, rl, min_mapq, thr = lib['orientation'], lib['read_len'], lib['min_mapq'], lib['ins_size_threshold']
    if mutate == 'floor_threshold':
        thr = math.floor(thr)
    detect = bool(lib['detect_duplicate'])
    twice = bool(lib['extend_paths']) and not lib['no_score']
    mask_a = MASK_GP if lib['no_score'] else (MASK_G | (MASK_GP if lib['extend_paths'] else 0))
    reach, accept, emit, dup, fishy = (np.zeros(n, bool) for _ in range(5))
    key = np.full(n, -1, np.int64)
    obs1, obs2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    aligned = [0] * nc
    count = non_unique = nus = n_dup = too_long = n_fishy = n_reach = 0
    prev = (-1, -1)
    tuples = []
    cols = [rec[k].tolist() if hasattr(rec[k], 'tolist') else rec[k] for k in ('tid', 'mtid', 'pos', 'mpos', 'flag', 'mapq', 'qlen')]
    for i, (t, m, pos, mpos, flag, mapq, qlen) in enumerate(zip(*cols)):
        if not (0 <= t < nc and 0 <= m < nc):
            continue
        if cls[t] == CLS_ABSENT or (cls[m] == CLS_ABSENT and mutate != 'coverage_with_absent_mate'):
            continue
        if mapq >= min_mapq or (mapq == 0 and mutate != 'mapq0_without_coverage'):
            aligned[t] += qlen
        if cls[m] == CLS_ABSENT:
            continue
        rdir, mdir = not (flag & F_REVERSE), not (flag & F_MREVERSE)
        if (flag & F_UNMAPPED) and (flag & F_READ1) and scaf[t] != scaf[m]:
            a = scaf[t] * 2 + posdir(fr, cdir[t], rdir, 0, 0, 0, 0, 0)[1]
            b = scaf[m] * 2 + posdir(fr, cdir[m], mdir, 0, 0, 0, 0, 0)[1]
            lo, hi = min(a, b), max(a, b)
            fishy[i] = True
            key[i] = (((lo << NODE_BITS) | hi) << 1) | 1
            n_fishy += 1
            tuples.append((lo, hi, 1, 0, 0, 0))
        if t != m and mapq == 0 and (mutate != 'non_unique_read2_only' or (flag & F_READ2)):
            non_unique += 1
        if not (t != m and (flag & F_READ2) and not (flag & F_UNMAPPED) and mapq >= min_mapq):
            continue
        if cls[t] == CLS_LARGE and cls[m] == CLS_LARGE and scaf[t] != scaf[m]:
            mask, calls = mask_a, (2 if twice else 1)
        elif lib['extend_paths'] and ((cls[t] == CLS_SMALL) != (cls[m] == CLS_SMALL) or
                                      (cls[t] == CLS_SMALL and cls[m] == CLS_SMALL and scaf[t] != scaf[m])):
            mask, calls = MASK_GP, 1
        else:
            continue
        o1, s1 = posdir(fr, cdir[t], rdir, cpos[t], pos, slen[t], clen[t], rl)
        o2, s2 = posdir(fr, cdir[m], mdir, cpos[m], mpos, slen[m], clen[m], rl)
        low = 24 if mutate == 'ge_25' else 25
        ok = (o1 + o2 <= thr if mutate == 'le_threshold' else o1 + o2 < thr) and o1 > low and o2 > low
        reach[i], accept[i], obs1[i], obs2[i] = True, ok, o1, o2
        n_reach += 1
        a, b = scaf[t] * 2 + s1, scaf[m] * 2 + s2
        lo, hi, o_lo, o_hi = (a, b, o1, o2) if a < b else (b, a, o2, o1)
        key[i] = ((lo << NODE_BITS) | hi) << 1
        kept = False
        for call in range(calls):
            if mapq == 0:
                nus += 1
            against = prev if (call == 0 or mutate == 'second_call_keeps_prev') else (-1, -1)
            same = o1 == against[0] and (o2 == against[1] or mutate == 'dup_on_o1_only')
            if same:
                n_dup += 1
                if call == 0:
                    dup[i] = True
                if detect:
                    if mutate == 'duplicate_still_calls_twice':
                        continue
                    break
            if ok:
                count += 1
                kept = True
            else:
                too_long += 1
            if mutate != 'prev_from_kept' or ok:
                prev = (o1, o2)
        if kept:
            emit[i] = True
            tuples.append((lo, hi, 0, o_lo, o_hi, mask))
    counters = [count, non_unique, nus, n_dup, too_long, n_fishy, len(tuples), n_reach, prev[0], prev[1]]
    return Replay(reach, accept, emit, dup, fishy, key, obs1, obs2, counters, aligned, prev, n_reach, tuples)


# ---- the census ------------------------------------------------------------------------------------------------------------
Census = collections.namedtuple(
    'Census', 'evaluable sub_counts queue_before ring_peak head_wraps round_of rounds chunks chunk_sizes chunk_keys '
              'candidates group_counts block_candidates ord_rounds heads dropped_heads')


def census(rec, lib, rp):
    """Where the records of a stream fall in the kernels' structures, from the rules the source comments state.  rp: the
    stream's Replay.
    evaluable: per record - `tid != mtid` and (mapped read 2 with mapq >= min_mapq, or unmapped read 1): what the fused loop
    queues.  sub_counts[b][s]: evaluable records of sub-tile s of block b.  queue_before[b][s]: candidates still queued when
    sub-tile s arrives - rounds take 64 at a time and a block ends with a short round, so it is the block's running count
    mod 64.  ring_peak: the largest queue_before + sub_counts.  head_wraps: sub-tiles whose candidates are written across
    the ring's end (the queue's head at 64 * rounds taken, mod the ring).  round_of: per evaluable record, its evaluation round
    within the block; rounds[b]: the sizes of block b's rounds.
    chunks[b] / chunk_sizes[b] / chunk_keys[b]: the chunks the run-grouping form closes in block b - in front of a round that
    emits, when kRlCloseRuns runs are open or the round's tuples would go past kRlChunkTuples; the block's first reaching
    record (its head) emits on its acceptance alone and is in no run - their tuple counts and their runs' keys.
    candidates: per record `tid != mtid` (the two-pass form); group_counts[b][g] per 256-record group, block_candidates[b],
    ord_rounds[b] = rounds of kOrdRound.  heads: per block the index of its first reaching record (-1: none);
    dropped_heads: those the stitch takes out again - accepted, but a duplicate of the last reaching record before the block."""
    tid, mtid, flag, mapq = (np.asarray(rec[k]).astype(np.int64) for k in ('tid', 'mtid', 'flag', 'mapq'))
    n = len(tid)
    nb = (n + BLOCK - 1) // BLOCK
    cand = tid != mtid
    link = ((flag & F_READ2) != 0) & ((flag & F_UNMAPPED) == 0) & (mapq >= lib['min_mapq'])
    quirk = ((flag & F_UNMAPPED) != 0) & ((flag & F_READ1) != 0)
    ev = cand & (link | quirk)

    def per(x, unit):
        pad = np.zeros(nb * BLOCK, np.int64)
        pad[:n] = x
        return pad.reshape(nb, BLOCK // unit, unit).sum(axis=2)
    sub_counts = per(ev, SUB)
    cum = np.cumsum(sub_counts, axis=1) - sub_counts
    queue_before = cum % 64
    ring_peak = int((queue_before + sub_counts).max(initial=0))
    q_head = (cum // 64 * 64) % RING
    head_wraps = [(int(b), int(s)) for b, s in zip(*np.nonzero((q_head + queue_before + sub_counts > RING) & (sub_counts > 0)))]
    round_of = np.full(n, -1, np.int64)
    rounds, chunks, chunk_sizes, chunk_keys, heads, dropped = [], [], [], [], [], []
    for b in range(nb):
        lo, hi = b * BLOCK, min(n, (b + 1) * BLOCK)
        idx = lo + np.nonzero(ev[lo:hi])[0]
        round_of[idx] = np.arange(len(idx)) // 64
        rounds.append([min(64, len(idx) - s) for s in range(0, len(idx), 64)])
        reaching = lo + np.nonzero(rp.reach[lo:hi])[0]
        head = int(reaching[0]) if len(reaching) else -1
        heads.append(head)
        if head >= 0 and rp.accept[head] and not rp.emit[head]:
            dropped.append(head)
        # the chunks: what a round emits is every fishy record, every kept link, and the head where it is accepted
        n_chunks, sizes, keys_of = 0, [], []
        open_n, open_keys = 0, set()
        for s in range(0, len(idx), 64):
            members = idx[s:s + 64]
            emitting = [int(i) for i in members if rp.fishy[i] or (rp.accept[i] if i == head else rp.emit[i])]
            if not emitting:
                continue
            if len(open_keys) >= K['kRlCloseRuns'] or open_n + len(emitting) > K['kRlChunkTuples']:
                if open_n:
                    n_chunks += 1
                    sizes.append(open_n)
                    keys_of.append(open_keys)
                open_n, open_keys = 0, set()
            open_n += len(emitting)
            open_keys = open_keys | {int(rp.key[i]) for i in emitting if i != head}
        if open_n:
            n_chunks += 1
            sizes.append(open_n)
            keys_of.append(open_keys)
        chunks.append(n_chunks)
        chunk_sizes.append(sizes)
        chunk_keys.append(keys_of)
    group_counts = per(cand, GROUP)
    block_candidates = group_counts.sum(axis=1)
    ord_rounds = [-(-int(c) // K['kOrdRound']) for c in block_candidates]
    return Census(ev, sub_counts, queue_before, ring_peak, head_wraps, round_of, rounds, chunks, chunk_sizes, chunk_keys, cand,
                  group_counts, block_candidates, ord_rounds, heads, dropped)


def slot_hash(key):
    """Where the run-grouping form starts probing for a key: (n_max + 5 n_min + 64 fishy) & (kRlSlots - 1)."""
    fishy, pair = key & 1, key >> 1
    return ((pair & ((1 << NODE_BITS) - 1)) + 5 * (pair >> NODE_BITS) + 64 * fishy) & (K['kRlSlots'] - 1)


# ---- building streams ------------------------------------------------------------------------------------------------------
class Builder(object):
    """n records, all of them fillers at first - a read 1 whose mate lies on the same contig, mapq 60, qlen 100: coverage and
    nothing else, the contig changing every 1000 records -, into which the designed records are put by index."""

    def __init__(self, n, lib, filler_rows=None):
        self.n, self.lib = n, lib
        rows = np.asarray(filler_rows if filler_rows is not None else rows_of('large')[:40], np.int32)
        self.tid = rows[(np.arange(n) // 1000) % len(rows)].astype(np.int32)
        self.mtid = self.tid.copy()
        self.pos = (np.arange(n, dtype=np.int64) % 5000).astype(np.int32)
        self.mpos = self.pos + 300
        self.flag = np.full(n, F_READ1 | F_MREVERSE | 1, np.uint16)
        self.mapq = np.full(n, 60, np.uint8)
        self.qlen = np.full(n, 100, np.uint16)
        self.wanted = {}                                     # record -> the observations it was placed for

    def link(self, i, row1, row2, o1, o2, reverse=False, mreverse=True, mapq=60, qlen=100, extra_flags=0):
        """Record i: a mapped read 2 on row1 with its mate on row2, placed to observe (o1, o2)."""
        self.tid[i], self.mtid[i] = row1, row2
        self.pos[i], self.mpos[i] = place(row1, reverse, o1, self.lib), place(row2, mreverse, o2, self.lib)
        self.flag[i] = 1 | F_READ2 | (F_REVERSE if reverse else 0) | (F_MREVERSE if mreverse else 0) | extra_flags
        self.mapq[i], self.qlen[i] = mapq, qlen
        self.wanted[int(i)] = (o1, o2)

    def raw(self, i, tid, mtid, flag, mapq=60, pos=100, mpos=150, qlen=100):
        self.tid[i], self.mtid[i], self.pos[i], self.mpos[i] = tid, mtid, pos, mpos
        self.flag[i], self.mapq[i], self.qlen[i] = flag, mapq, qlen

    def fishy(self, i, row1, row2, reverse=False, mreverse=False):
        """An unmapped read 1 with its mate on another scaffold (the BWA flag quirk, CreateGraph.py:141-163)."""
        self.raw(i, row1, row2, 1 | F_UNMAPPED | F_READ1 | (F_REVERSE if reverse else 0) | (F_MREVERSE if mreverse else 0))

    def idle(self, i, row1=None, row2=None):
        """An evaluable candidate that does not reach CreateEdge: a mapped read 2 whose mate is on the OTHER contig of its own
        scaffold."""
        a, b = rows_of('pair0')[3], rows_of('pair1')[3]
        self.raw(i, a if row1 is None else row1, b if row2 is None else row2, 1 | F_READ2 | F_MREVERSE)

    def records(self, n=None):
        n = self.n if n is None else n
        return dict(tid=self.tid[:n].copy(), mtid=self.mtid[:n].copy(), pos=self.pos[:n].copy(), mpos=self.mpos[:n].copy(),
                    flag=self.flag[:n].copy(), mapq=self.mapq[:n].copy(), qlen=self.qlen[:n].copy())


def distinct_obs(i):
    """Observations that differ between any two records less than 90 000 apart, both above 25, their sum below 700."""
    return 30 + i % 300, 30 + (i // 300) % 300


LARGE = rows_of('large')
SMALL = rows_of('small')
Stream = collections.namedtuple('Stream', 'name records lib claims')


# ---- rules -------------------------------------------------------------------------------------------------------------------
RULE_LIBS = [
    make_lib('fr', 100, 800.0, 11, True, True, False),       # the double call
    make_lib('rf', 100.38, 800.5, 0, True, True, False),     # min_mapq 0 with the double call: mapq 0 reaches CreateEdge
    make_lib('fr', 100.38, 800.0, 11, False, False, False),
    make_lib('rf', 100, 800.0, 0, False, True, True),
    make_lib('fr', 100, 800.5, 0, True, False, True),
    make_lib('rf', 100.38, 800.0, 11, True, True, True),
]


def rule_pairs():
    """(name, tid, mtid) for both contig directions of every pair kind."""
    nc = N_CONTIGS
    out = []
    for fwd in (True, False):
        lg, sm = rows_of('large', fwd), rows_of('small', fwd)
        p0, p1 = rows_of('pair0')[1 if fwd else 2], rows_of('pair1')[1 if fwd else 2]
        ab = rows_of('absent')[3 if fwd else 4]
        out += [('large/large', lg[0], lg[7]), ('large/small', lg[1], sm[2]), ('small/small', sm[3], sm[4]),
                ('*/absent', lg[2], ab), ('absent/*', ab, lg[3]), ('two contigs of a scaffold', p0 if fwd else p1, p1 if fwd else p0),
                ('same contig', lg[4], lg[4]), ('tid -1', -1, lg[5]), ('tid beyond', nc + (0 if fwd else 1000), lg[5]),
                ('mtid -1', lg[6], -1), ('mtid beyond', lg[6], nc + (0 if fwd else 77))]
    return out


def rules_stream(k):
    lib = RULE_LIBS[k]
    mq = lib['min_mapq']
    flags = [sum(bit for j, bit in enumerate((F_UNMAPPED, F_MUNMAPPED, F_REVERSE, F_MREVERSE, F_READ1, F_READ2)) if c >> j & 1)
             for c in range(64)]
    product = [(f, q, p) for p in rule_pairs() for q in (0, max(mq - 1, 0), mq, 255) for f in flags]
    order = list(range(len(product))) + list(np.random.default_rng(100 + k).permutation(len(product)))
    b = Builder(len(order), lib)
    for i, j in enumerate(order):
        f, q, (_, t, m) = product[j]
        b.raw(i, t, m, f | 1, mapq=q, pos=40 + (j * 7) % 311, mpos=45 + (j * 11) % 293, qlen=50 + j % 100)
    claims = dict(product=len(product), pair_kinds=sorted({p[0] for p in rule_pairs()}))
    return Stream('rules%d' % k, b.records(), lib, claims)


# ---- acceptance ----------------------------------------------------------------------------------------------------------------
def acceptance_stream(name, place_lib, run_lib=None):
    """Reaching records 8 apart whose observations are solved for: every pair of {-1, 0, 25, 26}, and sums one below, at and one
    above ceil(threshold), each through all sixteen pairs of calculator branches (two contig directions x two strands, both
    ends).  run_lib: the library the stream is run under when it is not the one it was placed for (the same coordinates
    through the float branches)."""
    run_lib = run_lib or place_lib
    T = int(math.ceil(place_lib['ins_size_threshold']))
    wanted = [(a, c) for a in (-1, 0, 25, 26) for c in (-1, 0, 25, 26)]
    wanted += [(26, T - 1 - 26), (26, T - 26), (26, T + 1 - 26), (300, T - 301), (300, T - 300), (300, T - 299), (T - 27, 26)]
    ends = [(LARGE_F, False), (LARGE_F, True), (LARGE_R, False), (LARGE_R, True)]
    combos = [(e1, e2) for e1 in ends for e2 in ends]
    b = Builder(8 * len(wanted) * len(combos) + 40, place_lib)
    placed = {}
    i = 5
    for c, ((rows1, rev1), (rows2, rev2)) in enumerate(combos):  # (no two neighbours observe the same: no duplicates here)
        for w, (o1, o2) in enumerate(wanted):
            b.link(i, rows1[(w + c) % 20], rows2[20 + (w * 3 + c) % 20], o1, o2, reverse=rev1, mreverse=rev2)
            placed[i] = (branch_of(place_lib, b.tid[i], rev1), branch_of(place_lib, b.mtid[i], rev2))
            i += 8
    claims = dict(observations=dict(b.wanted) if run_lib is place_lib else {}, threshold=T,
                  branches=sorted(set(placed.values())), placed=sorted(b.wanted))
    return Stream(name, b.records(), run_lib, claims)


LARGE_F, LARGE_R = rows_of('large', True), rows_of('large', False)


def acceptance_streams():
    whole, frac = make_lib(read_len=100, threshold=800.0), make_lib('rf', read_len=99.999, threshold=800.5)
    half = make_lib(read_len=0.5, threshold=800.5, extend_paths=False)
    return [acceptance_stream('accept_whole', whole), acceptance_stream('accept_fractional', frac),
            acceptance_stream('accept_half', half), acceptance_stream('accept_same_coordinates', whole, dict(whole, read_len=99.999))]


# ---- chain -----------------------------------------------------------------------------------------------------------------------
def chain_stream(detect):
    """Pairs of reaching records with equal observations (on different node pairs: a duplicate is a matter of observations
    alone), everything between them fillers unless said otherwise.  claims['pairs']: name -> (first, second)."""
    lib = make_lib(detect_duplicate=detect)                  # large/large links call CreateEdge twice
    n = 7 * BLOCK + 300
    b = Builder(n, lib)
    pairs = {}
    serial = [0]

    def obs():
        serial[0] += 1
        return distinct_obs(7 * serial[0])

    def pair(name, i, j, o=None, rows=None, third=None, **kw):
        o = o or obs()
        r = rows or (LARGE, LARGE)
        k = serial[0]
        b.link(i, r[0][k % 30], r[1][30 + k % 30], o[0], o[1], **kw)
        b.link(j, r[0][(k + 1) % 30], r[1][31 + k % 30], o[0], o[1], **kw)
        if third is not None:
            b.link(third, r[0][(k + 2) % 30], r[1][32 + k % 30], o[0], o[1], **kw)
        pairs[name] = (i, j) if third is None else (i, j, third)

    # block 0.  The stream's first reaching record observes (-1, -1): the initial prev_obs.
    b.link(2, LARGE[0], LARGE[40], -1, -1)
    pairs['first reaching record against the initial prev_obs'] = (2,)
    pair('next lane', 40, 44)
    pair('inside a lane', 80, 83)
    pair('chain of three', 120, 125, third=131)
    pair('predecessor reaches but is not accepted', 160, 166, o=(10, 400))
    pair('fishy record between', 200, 206)
    b.fishy(203, LARGE[3], LARGE[43])
    pair('small contig, one call', 240, 246, rows=(LARGE, SMALL))
    b.link(280, LARGE[5], LARGE[45], 77, 200)                # equal obs1, different obs2: no duplicate
    b.link(284, LARGE[6], LARGE[46], 77, 201)
    pairs['equal obs1 only'] = (280, 284)
    b.link(300, LARGE[7], LARGE[47], -1, -1)                 # the second call's prev_obs is (-1, -1)
    pairs['(-1, -1) under the double call'] = (300,)
    pair('sub-tile border', 2 * SUB - 1, 2 * SUB)
    # the 64th and 65th evaluable candidate of the block: 11 reaching records and a fishy one so far, from record 511 on
    # (evaluable so far: 2, 40, 44, 80, 83, 120, 125, 131, 160, 166, 200, 203, 206, 240, 246, 280, 284, 300, 511, 512 = 20)
    for j in range(43):
        b.idle(1000 + 3 * j)
    pair('round border', 1200, 1210)
    pair('block border', BLOCK - 1, BLOCK)                   # block 1: the head the stitch drops is the block's only tuple ...
    o = (int(b.wanted[BLOCK][0]), int(b.wanted[BLOCK][1]))
    # ... block 2 holds nothing that reaches; block 3's head repeats the observations again: a duplicate of a duplicate
    b.link(3 * BLOCK + 1, LARGE[9], LARGE[49], o[0], o[1])
    pairs['one block without a reaching record between'] = (BLOCK, 3 * BLOCK + 1)
    b.link(3 * BLOCK + 700, LARGE[10], LARGE[50], 90, 91)
    pair('three blocks without a reaching record between', 4 * BLOCK - 1, 7 * BLOCK + 2)
    b.link(7 * BLOCK + 200, LARGE[11], SMALL[3], 95, 96)
    claims = dict(pairs=pairs, blocks=8, only_tuple_block=1, empty_blocks=[2, 4, 5, 6], round_border=(1200, 1210),
                  dropped_heads=[BLOCK, 3 * BLOCK + 1, 7 * BLOCK + 2] if detect else [], observations=dict(b.wanted))
    return Stream('chain_%s' % ('detect' if detect else 'count'), b.records(), lib, claims)


# ---- ring --------------------------------------------------------------------------------------------------------------------------
RING_SUBS = [63, 256, 1, 0, 64, 65, 127, 128, 129, 255, 2, 63, 256]    # evaluable candidates of block 0's first sub-tiles
RING_LENGTHS = [2 * BLOCK, 2 * BLOCK + 1, 2 * BLOCK + 2, 2 * BLOCK + 3, 2 * BLOCK + SUB - 1, 2 * BLOCK + SUB, 2 * BLOCK + SUB + 1]


def _ring_builder():
    lib = make_lib('rf', read_len=100, min_mapq=0)
    b = Builder(3 * BLOCK, lib)

    def fill(first, count, every=1):
        for j in range(count):
            i = first + j * every
            if j % 3 == 2:
                b.idle(i)
            elif j % 17 == 5:
                b.fishy(i, LARGE[j % 20], LARGE[60 + j % 9])
            else:
                o = distinct_obs(i)
                b.link(i, LARGE[(i // 40) % 25], LARGE[50 + (i // 90) % 4], o[0], o[1], mapq=0 if j % 29 == 7 else 60)
    for s, c in enumerate(RING_SUBS):
        fill(s * SUB, c)
    fill(BLOCK - SUB, SUB)                                   # 256 candidates in the block's last sub-tile
    for i in range(BLOCK, 2 * BLOCK):                        # block 1: every record reaches
        o = distinct_obs(i)
        b.link(i, LARGE[(i // 700) % 25], LARGE[50 + (i // 2100) % 4], o[0], o[1])
    fill(2 * BLOCK, 300)                                     # block 2: the first sub-tile full, 44 in the second
    return b


def ring_streams():
    b = _ring_builder()
    out = []
    for n in RING_LENGTHS:
        claims = dict(ring_peak=RING - 1, n=n, all_reach_block=1, observations={i: o for i, o in b.wanted.items() if i < n})
        out.append(Stream('ring_n%d' % n, b.records(n), b.lib, claims))
    return out


# ---- runs ----------------------------------------------------------------------------------------------------------------------------
def _keyed(b, i, k):
    """A kept link at record i whose key is picked by k: LARGE[0] against LARGE[1 + k], or the two rows k names."""
    row1, row2 = k if isinstance(k, tuple) else (LARGE[0], LARGE[1 + k])
    o = distinct_obs(i)
    b.link(i, row1, row2, o[0], o[1])


def _round(b, first, keys, idle=0):
    """An evaluation round: records first .. first + 63, `idle` of them candidates that do not reach, the others links with
    the given key numbers (cycled)."""
    for j in range(64):
        if j < idle:
            b.idle(first + j)
        else:
            _keyed(b, first + j, keys[(j - idle) % len(keys)])


def _key_rounds_block(b, base, key_rounds):
    """A block that closes one chunk per round: its head alone in the first round (in no run), then rounds of 64 new keys - a
    round that finds 64 runs open closes the chunk."""
    _keyed(b, base, 200)
    for j in range(1, 64):
        b.idle(base + j)
    for r in range(key_rounds):
        _round(b, base + 64 * (r + 1), list(range(64)))


def runs_stream(over):
    """Blocks whose chunks close on purpose.  over: a block with one chunk more than the run tables hold (the pass is then
    repeated without run grouping).
    A round that finds kRlCloseRuns (64) runs open closes the chunk before it adds its own, so the fullest table there can be
    is 63 open runs and a round of 64 new keys: 127 of the 128 slots (block 1).  Block 2 is the other side of that rule:
    every round finds exactly 64 runs open and closes."""
    lib = make_lib(extend_paths=False)                       # one CreateEdge call per record
    b = Builder(4 * BLOCK + 77, lib)
    # block 0: rounds of 64 + 64 + .. + 63 + 1 tuples on three keys: a chunk of exactly 512 tuples; then, after a round
    # that closes it, the same with 2 tuples in the last round: 513 would not fit, the chunk closes at 511
    for r in range(7):
        _round(b, 64 * r, [0, 1, 2])
    _round(b, 64 * 7, [0, 1, 2], idle=1)
    _round(b, 64 * 8, [3], idle=63)                          # .. 512
    for r in range(9, 16):
        _round(b, 64 * r, [0, 1, 2])
    _round(b, 64 * 16, [0, 1, 2], idle=1)
    _round(b, 64 * 17, [3], idle=62)                         # 511 + 2
    _round(b, 64 * 18, [4, 5], idle=0)
    # block 1: 63 runs open in front of a round of 64 new keys (127 of the 128 slots in use), keys of one hash among them;
    # then a link key and the fishy key of the same node pair, and a run of one tuple among many
    base = BLOCK
    pool = [(r1, r2) for r1 in LARGE[500:520] for r2 in LARGE[600:900]]
    top = max(slot_hash(_key_of(lib, r1, r2)) for r1, r2 in pool)
    same_hash = [k for k in pool if slot_hash(_key_of(lib, *k)) == top][:8]
    assert len(same_hash) == 8 and top + 8 > K['kRlSlots']   # eight keys of one hash: their probing runs across the table's end
    others = list(range(400))
    first, second = (same_hash[:4] + others[:60]), (same_hash[4:] + others[60:120])
    _round(b, base, first[:63] + [first[0]], idle=0)         # the block's head is record `base`: 63 keys in runs
    _round(b, base + 64, second[:64])
    _round(b, base + 128, [0, 1])                            # closes the chunk of 127 keys
    b.fishy(base + 192, LARGE[0], LARGE[1], mreverse=True)   # same node pair as key 0 ...
    for j in range(1, 64):
        _keyed(b, base + 192 + j, 0 if j % 2 else 7)
    _keyed(b, base + 230, 300)                               # a run of one tuple
    # block 2: exactly kRlMaxChunks chunks (or one more)
    _key_rounds_block(b, 2 * BLOCK, K['kRlMaxChunks'] + (1 if over else 0))
    # block 3: a few tuples, and the stream's ragged end
    for j in range(40):
        _keyed(b, 3 * BLOCK + 5 * j, j % 3)
    claims = dict(chunk_512_block=0, table_127_block=1, chunks_block=2, chunks=K['kRlMaxChunks'] + (1 if over else 0),
                  fishy_pair_block=1, over=over, observations=dict(b.wanted))
    return Stream('runs_over' if over else 'runs', b.records(), lib, claims)


def _key_of(lib, row1, row2):
    """The key of a link between row1 and row2 as Builder.link makes it (forward read, reverse mate)."""
    a = TABLE['scaf'][row1] * 2 + posdir(lib['orientation'], TABLE['cdir'][row1], True, 0, 0, 0, 0, 0)[1]
    c = TABLE['scaf'][row2] * 2 + posdir(lib['orientation'], TABLE['cdir'][row2], False, 0, 0, 0, 0, 0)[1]
    return ((min(a, c) << NODE_BITS) | max(a, c)) << 1


# ---- groups ----------------------------------------------------------------------------------------------------------------------------
GROUP_BLOCK_CANDIDATES = [0, 1, K['kOrdRound'] - 1, K['kOrdRound'], K['kOrdRound'] + 1, 1023, 1024, 1025, 2049, BLOCK]


def groups_stream(short):
    """Blocks with 0, 1, one round (kOrdRound) - 1 / + 0 / + 1, 1023, 1024, 1025, 2049 and 16384 records whose mate is elsewhere
    (rounds of the two-pass form), groups
    with 0, 1, 255 and 256 of them, a block with candidates in its last group only, and an end one record behind (short: in
    front of) a stream tile's border, the last group not full."""
    lib = make_lib('rf', read_len=100.38, threshold=800.5, no_score=True)
    nb = len(GROUP_BLOCK_CANDIDATES) + 1
    n = nb * BLOCK + K['kStreamTile'] + (-1 if short else 1)
    b = Builder(n, lib)

    def cand(i, j):
        kind = j % 4
        if kind == 0:
            o = distinct_obs(i)
            b.link(i, LARGE[(i // 500) % 20], SMALL[(i // 900) % 20], o[0], o[1])
        elif kind == 1:
            b.raw(i, LARGE[(i // 500) % 20], LARGE[30], 1 | F_READ1 | F_REVERSE, mapq=0 if j % 8 == 1 else 30)   # read 1: non-unique at most
        elif kind == 2:
            b.idle(i)
        else:
            b.fishy(i, LARGE[(i // 500) % 20], SMALL[5 + j % 7])
    for blk, c in enumerate(GROUP_BLOCK_CANDIDATES):
        base = blk * BLOCK
        if c == BLOCK:
            for j in range(c):
                cand(base + j, j)
        elif c == 1:
            cand(base + 5 * GROUP + 17, 0)
        else:
            # group 1: 255, group 2: 256, group 3: 1 of them, the rest spread from group 8 on
            at = list(range(base + GROUP, base + 2 * GROUP - 1)) + list(range(base + 2 * GROUP, base + 3 * GROUP)) + [base + 3 * GROUP + 9]
            at = at[:c]
            rest = c - len(at)
            at += [base + 8 * GROUP + 5 * j for j in range(rest)]
            for j, i in enumerate(at):
                cand(i, j)
    last = len(GROUP_BLOCK_CANDIDATES) * BLOCK
    for j in range(30):                                      # candidates in the block's last group only
        cand(last + BLOCK - GROUP + 3 + 8 * j, j)
    for j, i in enumerate(range(n - 40, n)):                 # the ragged end
        cand(i, j)
    claims = dict(block_candidates=GROUP_BLOCK_CANDIDATES, last_group_only_block=len(GROUP_BLOCK_CANDIDATES), n=n,
                  observations=dict(b.wanted))
    return Stream('groups_short' if short else 'groups', b.records(), lib, claims)


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
def coverage_stream():
    lib = make_lib(min_mapq=11)
    n = 4 * BLOCK + 5
    b = Builder(n, lib)
    present = [r for r in range(N_CONTIGS) if TABLE['cls'][r] != CLS_ABSENT]
    absent = rows_of('absent')

    def own(i, row, mapq=60, qlen=100):
        b.raw(i, row, row, 1 | F_READ1 | F_MREVERSE, mapq=mapq, qlen=qlen)
    # block 0: the contig changes at a wave border, at a lane border and inside a lane's four records
    for i in range(0, SUB):
        own(i, present[1])
    for i in range(SUB, 2 * SUB + 4 * 9):
        own(i, present[2], qlen=101)
    for i in range(2 * SUB + 4 * 9, 3 * SUB + 4 * 20 + 2):
        own(i, present[3], qlen=102)
    for i in range(3 * SUB + 4 * 20 + 2, 4 * SUB):
        own(i, present[4], qlen=103)
    for j in range(600):                                     # one record per contig, absent ones among them
        own(4 * SUB + j, j, qlen=60 + j % 50)
    for j in range(300):                                     # runs of tid -1 and of ids beyond the table
        b.raw(7 * SUB + j, -1, -1, 1 | F_UNMAPPED | F_READ1, mapq=0)
        b.raw(9 * SUB + j, N_CONTIGS + j % 3, N_CONTIGS + j % 3, 1 | F_READ1, mapq=60)
    for j in range(40):                                      # absent contigs on either side of a candidate, of both kinds
        i = 11 * SUB + 6 * j
        flag = 1 | (F_READ2 if j % 2 else F_READ1) | F_MREVERSE
        b.raw(i, present[5 + j % 3], absent[j % 9], flag, mapq=(60, 0, 5)[j % 3], qlen=77)
        b.raw(i + 1, absent[j % 9], present[5 + j % 3], flag, mapq=(60, 0, 5)[j % 3], qlen=78)
        b.raw(i + 2, present[5 + j % 3], N_CONTIGS + 5, flag, mapq=(60, 0, 5)[j % 3], qlen=79)
    for j in range(200):                                     # mapq below min_mapq but not 0: no coverage
        own(13 * SUB + j, present[9], mapq=1 + j % 10, qlen=90)
        if j % 5 == 0:
            b.raw(13 * SUB + j, present[9], present[17], 1 | F_READ2 | F_MREVERSE, mapq=1 + j % 10, qlen=91)
    for j in range(20):                                      # mapq 0 counts for coverage whatever min_mapq is
        own(13 * SUB + 200 + j, present[9], mapq=0, qlen=33)
    # blocks 1 and 2: one contig, every read as long as the column holds: 16384 x 65535 per block, just below 2^30 in the
    # block's running sum and just below 2^31 on the contig
    for i in range(BLOCK, 3 * BLOCK):
        own(i, present[12], qlen=65535)
    big = present[12]
    claims = dict(big_contig=big, big_sum=2 * BLOCK * 65535, changes=[SUB, 2 * SUB + 36, 3 * SUB + 82])
    return Stream('coverage', b.records(), lib, claims)


# ---- all of them ---------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def all_streams():
    """name -> Stream, built once per process."""
    if not _CACHE:
        streams = [rules_stream(k) for k in range(len(RULE_LIBS))] + acceptance_streams() + \
            [chain_stream(True), chain_stream(False)] + ring_streams() + [runs_stream(False), runs_stream(True)] + \
            [groups_stream(False), groups_stream(True), coverage_stream()]
        for s in streams:
            assert s.name not in _CACHE
            _CACHE[s.name] = s
    return _CACHE


STREAM_NAMES = (['rules%d' % k for k in range(len(RULE_LIBS))] +
                ['accept_whole', 'accept_fractional', 'accept_half', 'accept_same_coordinates', 'chain_detect', 'chain_count'] +
                ['ring_n%d' % n for n in RING_LENGTHS] + ['runs', 'runs_over', 'groups', 'groups_short', 'coverage'])

# the stream on which each wrong rule shows
MUTATION_TARGETS = {
    'prev_from_kept': 'chain_detect', 'dup_on_o1_only': 'chain_detect', 'le_threshold': 'accept_whole', 'ge_25': 'accept_whole',
    'floor_threshold': 'accept_fractional', 'second_call_keeps_prev': 'chain_detect', 'duplicate_still_calls_twice': 'chain_detect',
    'coverage_with_absent_mate': 'coverage', 'mapq0_without_coverage': 'coverage', 'non_unique_read2_only': 'rules0',
}


def as_batch(stream):
    """The stream as a RecordBatch (tlen is not read by the record loop)."""
    from besst_amd.records import RecordBatch
    rec = stream.records
    names = ['c%d' % i for i in range(N_CONTIGS)]
    return RecordBatch(names, TABLE['clen'], tlen=np.zeros(len(rec['tid']), np.int32), **rec)


def as_oracle_inputs(stream):
    """(rec lists, table, LibParams) for oracle.py_oracle.record_loop."""
    from oracle import py_oracle as O
    rec = {k: v.tolist() for k, v in stream.records.items()}
    lib = stream.lib
    p = O.LibParams(orientation=lib['orientation'], read_len=lib['read_len'], ins_size_threshold=lib['ins_size_threshold'],
                    min_mapq=lib['min_mapq'], detect_duplicate=lib['detect_duplicate'], extend_paths=lib['extend_paths'],
                    no_score=lib['no_score'])
    return rec, TABLE, p
